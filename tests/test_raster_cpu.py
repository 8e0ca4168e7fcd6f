"""The restatement of the mesh rasteriser (tests/raster_numpy.py, the definition of csrc/raster.hip) against first principles, on
the CPU: watertightness of the fill rule on a closed sphere (every covered pixel receives exactly two fragments, exactly one
with back-face culling), orientation, exact coverage of a pixel-aligned quad, the depth of a tilted plane within a derived
bound, the tie rules, colours, and mesh.keep_faces (torch plumbing, no kernel) against its restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402
import raster_numpy as N                                 # noqa: E402
import warp_numpy as Wn                                  # noqa: E402

H, W, FOCAL = 48, 64, 60.0
# (angles, origin), pixels covered, fragments per covered pixel with cull 'none' / 'back'
SPHERE_POSES = (
    (((0., 0., 0.), (0., 0., 3.)), 481, 2, 1),
    (((.1, .5, .05), (1.6, -.3, 2.6)), 450, 2, 1),
    (((0., 0., 0.), (0., 0., .3)), H * W, 1, 0),          # the camera inside the sphere
)
IDENTITY = Wn.pose()

_cache = {}


def sphere():
    if 'sphere' not in _cache:
        v, f, _ = M.marching_cubes(R.lattice(24, R.sphere_field()), 1.0, R.LO, R.HI)
        v.setflags(write=False)
        f.setflags(write=False)
        _cache['sphere'] = (v, f)
    return _cache['sphere']


def view(i, cull):
    key = ('view', i, cull)
    if key not in _cache:
        v, f = sphere()
        (ang, org), *_ = SPHERE_POSES[i]
        _cache[key] = N.rasterize_view(v, f, Wn.pose(ang, org), H, W, FOCAL, cull=cull)
    return _cache[key]


def test_the_sphere_is_the_one_the_counts_were_measured_on():
    v, f = sphere()
    assert v.shape == (888, 3) and f.shape == (1772, 3) and M.is_closed(f)


@pytest.mark.parametrize('i', range(3))
def test_fill_rule_is_watertight_on_the_closed_sphere(i):
    _, covered, per_none, per_back = SPHERE_POSES[i]
    none, back = view(i, 'none'), view(i, 'back')
    hit = none['face'] >= 0
    assert int(hit.sum()) == covered
    # a closed surface seen from outside: one front and one back fragment on every covered pixel, none elsewhere -- a fill
    # rule that counts a shared edge twice, or not at all, gives 3 or 1 somewhere
    assert np.all(none['fragments'][hit] == per_none) and np.all(none['fragments'][~hit] == 0)
    if per_back:
        assert np.all(back['fragments'][hit] == per_back) and np.all(back['fragments'][~hit] == 0)
        assert np.array_equal(none['disp'].view(np.uint32), back['disp'].view(np.uint32))
        assert np.array_equal(none['face'], back['face'])
    else:                                                  # from inside every face is back-facing
        assert not back['fragments'].any() and np.all(back['face'] == -1) and np.all(back['disp'] == 0)
        assert not none['front'].any()
    assert np.all((none['disp'] > 0) == hit) and np.all(none['disp'][~hit] == 0)


@pytest.mark.parametrize('i', range(2))
def test_culled_winners_face_the_camera(i):
    v, f = sphere()
    (ang, org), *_ = SPHERE_POSES[i]
    back = view(i, 'back')
    winners = np.unique(back['face'][back['face'] >= 0])
    p = v.astype(np.float64)[f[winners]]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert len(winners) > 100 and np.all(np.einsum('ij,ij->i', n, np.asarray(org) - p.mean(1)) > 0)
    assert np.all(back['front'][winners])                  # A2 < 0 is front-facing


def quad():
    """a fronto-parallel quad at depth 3 whose corners project onto the pixels (12, 4), (52, 4), (52, 44), (12, 44)."""
    v = np.array([[-1, 1, -3], [1, 1, -3], [1, -1, -3], [-1, -1, -3]], np.float32)
    return v, np.array([[0, 2, 1], [0, 3, 2]])


def test_pixel_aligned_quad_covers_its_half_open_rectangle_once():
    v, f = quad()
    X, Y, d, ok = N.project(v, IDENTITY, H, W, FOCAL, 1e-3)
    assert ok.all() and X.tolist() == [12 * 256, 52 * 256, 52 * 256, 12 * 256] and Y.tolist() == [4 * 256, 4 * 256, 44 * 256, 44 * 256]
    for faces in (f, f[:, [0, 2, 1]], f[::-1]):            # either winding, either order
        r = N.rasterize_view(v, faces, IDENTITY, H, W, FOCAL)
        want = np.zeros((H, W), np.int64)
        want[4:44, 12:52] = 1                              # the left and top edges are in, the right and bottom ones out
        assert np.array_equal(r['fragments'], want)        # so the pixels on the shared diagonal belong to exactly one face
        assert set(np.unique(r['face'][4:44, 12:52])) == {0, 1}
        third = np.float32(1.0 / 3.0)
        got = r['disp'][4:44, 12:52]
        assert np.all(np.abs(got.view(np.int32).astype(np.int64) - int(third.view(np.int32))) <= 1)


def test_tilted_plane_depth_within_the_snapping_bound():
    """The rasteriser interpolates the exact vertex disparities over the SNAPPED vertex positions.  Disparity is affine on the
    screen, D(u, w) = gu u + gw w + c, so the interpolant D' is affine too and g = D' - D is affine with, at a snapped vertex
    s_k of the true vertex p_k, g(s_k) = D(p_k) - D(s_k) = -grad D . (s_k - p_k), |s_k - p_k| <= 2^-9 sqrt(2) pixels (half a
    sub-pixel step per axis).  Every covered pixel lies in the snapped triangle, where an affine function is bounded by its
    vertex values: |D' - D| <= |grad D| 2^-9 sqrt(2), plus the rounding of D' to fp32 (2^-24 relative)."""
    v = np.array([[-1.31, -1.1, -2.03], [1.47, -0.93, -4.0], [0.13, 1.4, -3.1]], np.float32)       # off the sub-pixel lattice
    r = N.rasterize_view(v, np.array([[0, 1, 2]]), IDENTITY, H, W, FOCAL)
    hit = r['face'] == 0
    assert hit.sum() > 500
    p = v.astype(np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    k = n @ p[0]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    analytic = (n[0] * (x - W / 2) / FOCAL - n[1] * (y - H / 2) / FOCAL - n[2]) / k
    grad = np.hypot(n[0] / (FOCAL * k), n[1] / (FOCAL * k))
    bound = grad * 2.0 ** -9 * np.sqrt(2.0) + analytic[hit].max() * 2.0 ** -24
    err = np.abs(r['disp'].astype(np.float64) - analytic)[hit].max()
    print(f'tilted plane: max |D - analytic| = {err:.3e}, bound {bound:.3e}')
    assert err <= bound and grad > 1e-3                    # a plane that is tilted indeed


def test_coincident_faces_go_to_the_lower_index():
    v = np.array([[-1, 1, -3], [1, 1, -3], [0, -1, -3]], np.float32)
    r = N.rasterize_view(v, np.array([[0, 2, 1], [0, 2, 1], [0, 2, 1]]), IDENTITY, H, W, FOCAL)
    hit = r['face'] >= 0
    assert hit.sum() > 300 and np.all(r['face'][hit] == 0) and np.all(r['fragments'][hit] == 3)


def overlap_mesh():
    """a small triangle at depth 2 in front of a large one at depth 4, and a third one behind both."""
    v = np.array([[-2, 1.5, -4], [2, 1.5, -4], [0, -1.5, -4], [-.3, .3, -2], [.3, .3, -2], [0, -.3, -2],
                  [-1, 1, -6], [1, 1, -6], [0, -1, -6]], np.float32)
    return v, np.array([[0, 2, 1], [3, 5, 4], [6, 8, 7]])


def test_nearest_wins_in_any_face_order():
    v, f = overlap_mesh()
    base = N.rasterize_view(v, f, IDENTITY, H, W, FOCAL)
    assert {0, 1} <= set(np.unique(base['face'])) and 2 not in base['face']       # the far one is hidden entirely
    near = base['face'] == 1
    assert near.sum() > 50 and np.all(base['disp'][near] == np.float32(0.5)) and np.all(base['fragments'][near] == 3)
    for perm in ([2, 1, 0], [1, 2, 0], [0, 2, 1]):
        r = N.rasterize_view(v, f[perm], IDENTITY, H, W, FOCAL)
        assert np.array_equal(r['disp'].view(np.uint32), base['disp'].view(np.uint32))
        hit = r['face'] >= 0
        assert np.array_equal(hit, base['face'] >= 0) and np.array_equal(np.asarray(perm)[r['face'][hit]], base['face'][hit])


def test_constant_colours_come_back_unchanged_and_interpolation_is_perspective_correct():
    v, f = sphere()
    col = np.tile(np.array([[10, 200, 77]], np.uint8), (len(v), 1))
    P = Wn.pose(*SPHERE_POSES[1][0])
    r = N.rasterize_view(v, f, P, H, W, FOCAL, colors=col)
    hit = r['face'] >= 0
    assert np.all(r['rgb'][hit] == [10, 200, 77]) and np.all(r['rgb'][~hit] == 0)
    # a colour that is affine in WORLD space must come back affine in world space (not in screen space): the tilted plane
    tv = np.array([[-1.3, -1.1, -2.0], [1.5, -0.9, -4.0], [0.1, 1.4, -3.0]], np.float32)
    tc = np.array([[0, 0, 0], [250, 0, 0], [0, 250, 0]], np.uint8)
    t = N.rasterize_view(tv, np.array([[0, 1, 2]]), IDENTITY, H, W, FOCAL, colors=tc)
    ys, xs = np.nonzero(t['face'] == 0)
    depth = 1.0 / t['disp'][ys, xs].astype(np.float64)
    pts = depth[:, None] * np.stack([(xs - W / 2) / FOCAL, -(ys - H / 2) / FOCAL, -np.ones(len(xs))], -1)
    A = np.concatenate([tv.astype(np.float64), np.ones((3, 1))], 1)               # colour = [x y z 1] . coef through the vertices
    A = np.concatenate([A, [[*np.cross(tv[1] - tv[0], tv[2] - tv[0]), 0.0]]])      # and constant along the normal
    coef = np.linalg.solve(A, np.concatenate([tc[:, :2].astype(np.float64), [[0.0, 0.0]]]))
    want = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ coef
    # rounding to a byte (0.5), plus snapping: 250 levels across a triangle whose altitudes exceed 20 pixels is under 12.5
    # levels per pixel, times the 2^-9 sqrt(2) pixels a vertex moves
    err = np.abs(t['rgb'][ys, xs, :2].astype(np.float64) - want).max()
    print(f'colour against the world-space affine function: max error {err:.4f} levels')
    assert err <= 0.5 + 12.5 * 2.0 ** -9 * np.sqrt(2.0)


def test_dropped_faces_and_bad_indices():
    v = np.array([[-1, 1, -3], [1, 1, -3], [0, -1, -3],           # 0-2 in front
                  [-1, 1, 3], [1, 1, 3], [0, -1, 3],              # 3-5 behind the camera
                  [0, -1, 0.5],                                   # 6: with 0, 1 a face that straddles z = near
                  [3000, 1, -3],                                  # 7: 60,000 pixels to the right: beyond the guard band
                  [0, 1, -3]], np.float32)                        # 8: on the edge 0-1: a zero-area face with 0, 1
    empty = N.rasterize_view(v, np.array([[3, 5, 4], [0, 6, 1], [0, 2, 7], [0, 8, 1]]), IDENTITY, H, W, FOCAL)
    assert not empty['fragments'].any() and np.all(empty['face'] == -1)
    one = N.rasterize_view(v, np.array([[3, 5, 4], [0, 6, 1], [0, 2, 1], [0, 2, 7], [0, 8, 1]]), IDENTITY, H, W, FOCAL)
    assert set(np.unique(one['face'])) == {-1, 2}
    for bad in ([[0, 1, 9]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match='outside'):
            N.rasterize_view(v, np.array(bad), IDENTITY, H, W, FOCAL)


def test_keep_faces_renumbers():
    from mvip_nerf_amd import mesh
    v, f = sphere()
    rs = np.random.RandomState(3)
    keep = rs.rand(len(f)) < 0.3
    nrm, col = rs.randn(len(v), 3).astype(np.float32), rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    rv, rf, rn, rc = N.keep_faces(v, f, keep, nrm, col)
    assert 0 < len(rv) < len(v) and rf.min() == 0 and rf.max() == len(rv) - 1
    assert np.array_equal(rv[rf], v[f[keep]])              # the same triangles, in the same order
    assert np.all(np.diff(np.nonzero(np.isin(np.arange(len(v)), f[keep]))[0]) > 0)
    m = mesh.Mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.astype(np.int32)), torch.from_numpy(nrm), torch.from_numpy(col))
    out = mesh.keep_faces(m, torch.from_numpy(keep))
    assert out.faces.dtype == torch.int32 and out.verts.dtype == torch.float32 and out.colors.dtype == torch.uint8
    for got, want in zip(out, (rv, rf, rn, rc)):
        assert np.array_equal(got.numpy(), want)
    bare = mesh.keep_faces(mesh.Mesh(m.verts, m.faces, None, None), torch.zeros(len(f), dtype=torch.bool))
    assert bare.verts.shape == (0, 3) and bare.faces.shape == (0, 3) and bare.normals is None and bare.colors is None
    with pytest.raises(ValueError, match='keep'):
        mesh.keep_faces(m, torch.zeros(3, dtype=torch.bool))
