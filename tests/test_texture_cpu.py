"""The restatement of the mesh texturing (tests/texture_numpy.py, the definition of csrc/texture.hip) against first principles: the
atlas layout's ownership property, an affine image on a plane, occlusion and the four-pixel rule, masks, the cos^2 weights, the
edges of the image, the OBJ export, and what a texture carries that vertex colours cannot.  No GPU."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402
import raster_numpy as N                                 # noqa: E402
import texture_numpy as T                                # noqa: E402
import warp_numpy as Wn                                  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvip_nerf_amd import mesh                           # noqa: E402

H, W, FOCAL = 48, 64, 60.0
IDENTITY = Wn.pose()
F64, I64 = np.float64, np.int64


def pixel_point(u, w, z, focal=FOCAL):
    """the world point that the identity camera sees at pixel (u, w) and planar depth z."""
    return [(u - W / 2) * z / focal, -(w - H / 2) * z / focal, -z]


def quad(x0, y0, x1, y1, z):
    """two faces over the pixel rectangle [x0, x1] x [y0, y1] of the identity camera at depth z, counter-clockwise seen from it."""
    v = np.asarray([pixel_point(x0, y0, z), pixel_point(x0, y1, z), pixel_point(x1, y1, z), pixel_point(x1, y0, z)], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# ---- 1. the layout ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 2, 3, 8, 32])
@pytest.mark.parametrize('F', [1, 2, 7, 1772])
def test_layout_owner_map_and_footprints(F, n):
    L = T.layout(F, n)
    S, Bx = L['S'], L['Bx']
    face, hi, hj = T.owner_map(F, n)
    assert face.shape == (L['Ht'], L['Wt']) and Bx * Bx >= (F + 1) // 2 > (Bx - 1) * (Bx - 1) and L['By'] == -(-((F + 1) // 2) // Bx)
    # total over the used halves, disjoint (the map is single-valued) and nothing else owned
    counts = np.bincount(face[face >= 0], minlength=F)
    want = np.where(np.arange(F) % 2 == 0, S * (S + 1) // 2, S * (S - 1) // 2)
    assert np.array_equal(counts, want) and counts.sum() + int((face < 0).sum()) == face.size
    if F % 2:                                               # the second half of the last block has no owner
        k = F // 2
        block = face[(k // Bx) * S:(k // Bx + 1) * S, (k % Bx) * S:(k % Bx + 1) * S]
        assert set(np.unique(block)) == {F - 1, -1} and int((block < 0).sum()) == S * (S - 1) // 2
    # ownership seen from the other side: the texel sets written from the halves' own coordinates
    f = np.arange(F, dtype=I64)
    bx, by, upper = (f // 2) % Bx, (f // 2) // Bx, f % 2 == 1

    def texel(i, j):                                        # texture coordinates of (i, j) of every face's half
        return np.where(upper, bx * S + S - 1 - i, bx * S + i), np.where(upper, by * S + S - 1 - j, by * S + j)

    # bilinear footprints of UV points inside the closed UV triangle, in exact integer arithmetic: the point with barycentrics
    # (r, s) / m lies at a = n r / m, b = n s / m texels from the corner; a texel has non-zero weight iff it is floor(a), or
    # floor(a) + 1 with a fractional a (likewise b).  Corners, the three edges and the interior are all among (r, s).
    reach = 0
    for m in ((n, 2 * n + 1, 7) if F <= 7 else (n, 5)):
        for r in range(m + 1):
            for s in range(m + 1 - r):
                ia, ib = (n * r) // m, (n * s) // m
                for di in ((0, 1) if (n * r) % m else (0,)):
                    for dj in ((0, 1) if (n * s) % m else (0,)):
                        X, Y = texel(ia + di, ib + dj)
                        assert np.array_equal(face[Y, X], f), (m, r, s, di, dj)
                        reach = max(reach, ia + di + ib + dj)
    assert reach <= n + 1                                   # the halves meet at n + 2 | n + 3
    # the UV corners: continuous texel coordinates (1/2, 1/2), (n + 1/2, 1/2), (1/2, n + 1/2) of the half, in OBJ convention
    shape, uv = T.atlas_uv(F, n)
    assert shape == (L['Ht'], L['Wt'], 3) and uv.shape == (F, 3, 2) and uv.dtype == np.float32
    for c, (i, j) in enumerate(((0, 0), (n, 0), (0, n))):
        X, Y = texel(i, j)
        assert np.allclose(uv[:, c, 0] * L['Wt'], X + 0.5, atol=2e-3) and np.allclose((1 - uv[:, c, 1]) * L['Ht'], Y + 0.5, atol=2e-3)
    assert uv.min() >= 0 and uv.max() <= 1
    shape2, uv2 = mesh.atlas_layout(F, n)                   # the package's host code states the same layout
    assert shape2 == shape and uv2.dtype == np.float32 and np.array_equal(uv2, uv)


@pytest.mark.parametrize('n', [1, 2, 3, 8, 32])
@pytest.mark.parametrize('F', [1, 2, 7, 1772])
def test_layout_sample_points_lie_on_the_closed_face(F, n):
    rs = np.random.RandomState(F + n)
    verts = rs.uniform(-1, 1, (3 * F, 3)).astype(np.float32)
    faces = rs.permutation(3 * F).reshape(F, 3).astype(np.int32)
    face, p, nrm, (l0, l1, l2) = T.atlas_points(verts, faces, n)
    _, i, j = T.owner_map(F, n)
    own = face >= 0
    assert (l0[own] >= 0).all() and (l1[own] >= 0).all() and (l2[own] >= 0).all()
    assert np.abs((l0 + l1 + l2)[own] - 1).max() <= 4e-16
    inner = own & (i + j <= n)                              # the barycentric lattice, hypotenuse included
    assert np.abs(l1[inner] - i[inner] / n).max() <= 2e-16 and np.abs(l2[inner] - j[inner] / n).max() <= 2e-16
    assert np.abs(l0[inner] - (n - i - j)[inner] / n).max() <= 4e-16
    gutter = own & (i + j > n)                              # on the hypotenuse, between its end points
    assert (l0[gutter] == 0).all() and gutter.sum() > 0
    v64 = verts.astype(F64)
    for c, (ci, cj) in enumerate(((0, 0), (n, 0), (0, n))):  # the three corner texels ARE the three vertices
        sel = own & (i == ci) & (j == cj)
        assert sel.sum() == F and np.array_equal(p[sel], v64[faces[face[sel], c]])
    fv = v64[faces[face[own]]]
    exact = l0[own][:, None] * fv[:, 0] + l1[own][:, None] * fv[:, 1] + l2[own][:, None] * fv[:, 2]
    assert np.abs(p[own] - exact).max() <= 1e-15
    assert np.array_equal(nrm[own], np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]))
    with pytest.raises(ValueError, match='face index'):
        T.atlas_points(verts, [[0, 1, 3 * F]], n)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            T.layout(F, bad)
    with pytest.raises(ValueError, match='over 16384'):
        T.layout(2 * 2341 ** 2 + 1, 4)                      # 2,342 blocks of 7 per row: 16,394 texels


# ---- 2. an affine image on a plane ------------------------------------------------------------------------------------------------

AFFINE = ((10, 1, 1), (200, -1, -1), (5, 0, 2))            # value = a + b x + c y per channel: integers at the pixels, 0..255


def affine_image():
    y, x = np.mgrid[0:H, 0:W]
    im = np.stack([a + b * x + c * y for a, b, c in AFFINE], -1)
    assert im.min() >= 0 and im.max() <= 255
    return im.astype(np.uint8)


def test_affine_image_on_a_fronto_parallel_quad():
    """The quad's edges lie about half a pixel off the pixel centres (at positions chosen so that no texel's exact colour is a
    half-integer), so its pixels 10..30 x 8..28 are covered; at n = 32 a texel is 0.65 of a pixel.  Bilinear interpolation
    reproduces affine data, so a seen texel holds the affine function at its own projection, rounded.  The map between image and texture is affine for this pose, so the textured render reproduces the image
    too: within the rounding of the texels (1/2 level), of the output (1/2) and, next to the diagonal, the gutter texels, which
    hold the colour of the nearest point ON the hypotenuse and not the affine continuation past it (weight <= 1/4, displacement
    half a texel along each axis: under 1/4 level here) -- within 1 level in all."""
    n = 32
    v, f = quad(9.55, 7.45, 30.35, 28.4, 4.0)
    img = affine_image()[None]
    disp, fmap, _ = N.rasterize(v, f, IDENTITY[None], H, W, FOCAL)
    assert np.array_equal(np.nonzero((fmap[0] >= 0).any(0))[0], np.arange(10, 31)) and N.rasterize(v, f, IDENTITY[None], H, W, FOCAL, cull='back')[1].max() == 1
    rgb, wsum, best = T.bake_atlas(v, f, n, img, disp, IDENTITY[None], FOCAL)
    face, p, _, _ = T.atlas_points(v, f, n)
    u, w, _ = T.project_point(p.reshape(-1, 3), IDENTITY, H, W, FOCAL)
    exact = np.stack([a + b * u + c * w for a, b, c in AFFINE], -1).reshape(rgb.shape)
    seen = wsum > 0
    assert np.array_equal(seen, best == 0) and not seen[face < 0].any()
    assert seen.sum() > 0.8 * (face >= 0).sum()
    assert np.abs(exact[seen] - np.floor(exact[seen]) - 0.5).min() > 1e-6          # no value within 1e-6 of a half-integer
    assert np.array_equal(rgb[seen], np.floor(exact[seen] + 0.5).astype(np.uint8))
    assert (rgb[~seen] == 0).all()
    # a texel is unseen only where its footprint leaves the covered pixels: within one pixel of the quad's outline
    uu, ww = u.reshape(face.shape), w.reshape(face.shape)
    inside = (face >= 0) & (uu >= 10) & (uu <= 30) & (ww >= 8) & (ww <= 28)
    assert np.array_equal(seen, inside)
    _, fm, out = T.render_textured(v, f, rgb, n, IDENTITY[None], H, W, FOCAL)
    ys, xs = np.nonzero(fm[0] >= 0)
    keep = (xs >= 11) & (xs <= 29) & (ys >= 9) & (ys <= 27)                       # at least one pixel inside the quad
    assert keep.sum() == 19 * 19
    err = np.abs(out[0, ys[keep], xs[keep]].astype(int) - img[0, ys[keep], xs[keep]].astype(int))
    print(f'affine plane: {int(seen.sum())} of {int((face >= 0).sum())} owned texels seen; textured render max |error| {err.max()} level, '
          f'exact at {float((err == 0).mean()):.3f} of {err.size} pixel channels')
    assert err.max() <= 1


# ---- 3. occlusion -----------------------------------------------------------------------------------------------------------------

def two_quads():
    """a rear quad at depth 4 (faces 0, 1) and a smaller one in front of its middle at depth 2 (faces 2, 3), placed so that at 16
    texels per leg a column and a row of the rear quad's texel lattice have footprints across the front quad's silhouette."""
    rv, rf = quad(6.5, 4.5, 57.5, 43.5, 4.0)
    fv, ff = quad(22.6, 14.6, 43.5, 35.5, 2.0)
    return np.concatenate([rv, fv]), np.concatenate([rf, ff + 4]).astype(np.int32)


def oblique_pose():
    """a camera to the right of the identity camera, turned towards the quads: it sees the rear quad behind the front one."""
    return Wn.pose((0.0, 0.55, 0.0), (2.2, 0.0, 0.3))


def occlusion_scene(seed=5):
    v, f = two_quads()
    poses = np.stack([IDENTITY, oblique_pose()])
    images = np.random.RandomState(seed).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    disp, fmap, _ = N.rasterize(v, f, poses, H, W, FOCAL)
    return v, f, poses, images, disp, fmap


def footprints(p, pose):
    """(inside [N] bool, ys [N, 4], xs [N, 4]): the four footprint pixels of fp64 points p in a view, from the definition."""
    u, w, z = T.project_point(p, pose, H, W, FOCAL)
    with np.errstate(invalid='ignore'):
        inside = (z >= 1e-3) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
    x0, y0 = np.floor(np.where(inside, u, 0)).astype(int), np.floor(np.where(inside, w, 0)).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    return inside, np.stack([y0, y0, y1, y1], -1), np.stack([x0, x1, x0, x1], -1)


def test_occlusion_and_the_four_pixel_rule():
    n = 16
    v, f, poses, images, disp, fmap = occlusion_scene()
    rgb, wsum, best, wts = T.bake_atlas(v, f, n, images, disp, poses, FOCAL, details=True)
    face, p, _, _ = T.atlas_points(v, f, n)
    rear = (face == 0) | (face == 1)
    pts = p.reshape(-1, 3)
    inside, ys, xs = footprints(pts, poses[0])
    winners = fmap[0][ys, xs].reshape(face.shape + (4,))                              # the faces at the four footprint pixels
    hidden = rear & (winners >= 2).all(-1)                                           # wholly behind the front quad
    straddle = rear & (winners >= 2).any(-1) & (winners < 2).any(-1) & (winners >= 0).all(-1)
    clear = rear & np.isin(winners, (0, 1)).all(-1)
    assert hidden.sum() > 20 and straddle.sum() > 4 and clear.sum() > 100
    assert (wts[0][hidden] == 0).all()                      # the frontal view gives the hidden texels nothing
    assert (wts[0][straddle] == 0).all()                    # nor those whose footprint straddles the front quad's silhouette,
    u0, w0, _ = T.project_point(pts, poses[0], H, W, FOCAL)
    nearest = fmap[0][np.rint(np.where(inside, w0, 0)).astype(int), np.rint(np.where(inside, u0, 0)).astype(int)].reshape(face.shape)
    assert (nearest[straddle] < 2).any()                    # although the rear quad itself is what the nearest pixel shows
    assert (wts[0][clear] > 0).all()
    # the oblique view sees some of the hidden texels: it alone supplies their colour, and `best` names it
    from_oblique = hidden & (wts[1] > 0)
    assert from_oblique.sum() > 10
    assert (best[from_oblique] == 1).all() and (wsum[from_oblique] == wts[1][from_oblique].astype(np.float32)).all()
    only1 = T.bake_atlas(v, f, n, images[1:], disp[1:], poses[1:], FOCAL)[0]
    assert np.array_equal(rgb[from_oblique], only1[from_oblique]) and rgb[from_oblique].any()
    nobody = rear & (wts[0] == 0) & (wts[1] == 0)
    assert (best[nobody] == -1).all() and (wsum[nobody] == 0).all() and (rgb[nobody] == 0).all()
    # best = the view of largest weight everywhere
    both = (wts > 0).all(0)
    assert both.sum() > 100 and np.array_equal(best[both], np.argmax(wts[:, both], 0).astype(np.int32))
    best_mode = T.bake_atlas(v, f, n, images, disp, poses, FOCAL, mode='best')
    only0 = T.bake_atlas(v, f, n, images[:1], disp[:1], poses[:1], FOCAL)[0]
    assert np.array_equal(best_mode[2], best) and np.array_equal(best_mode[1], wsum)
    assert np.array_equal(best_mode[0][best == 0], only0[best == 0]) and np.array_equal(best_mode[0][best == 1], only1[best == 1])


def test_masks_remove_exactly_the_views_whose_footprint_touches_a_false_pixel():
    n = 16
    v, f, poses, images, disp, _ = occlusion_scene()
    masks = np.random.RandomState(8).uniform(size=(2, H, W)) > 0.15
    base = T.bake_atlas(v, f, n, images, disp, poses, FOCAL, details=True)[3]
    got = T.bake_atlas(v, f, n, images, disp, poses, FOCAL, masks=masks, details=True)[3]
    face, p, _, _ = T.atlas_points(v, f, n)
    for k in range(2):
        _, ys, xs = footprints(p.reshape(-1, 3), poses[k])
        free = masks[k][ys, xs].all(-1).reshape(face.shape)
        assert np.array_equal(got[k], np.where(free, base[k], 0.0))
        assert ((base[k] > 0) & ~free).sum() > 50 and ((base[k] > 0) & free).sum() > 50
    assert np.array_equal(T.bake_atlas(v, f, n, images, disp, poses, FOCAL, masks=np.ones_like(masks))[0],
                          T.bake_atlas(v, f, n, images, disp, poses, FOCAL)[0])


# ---- 4. weights -------------------------------------------------------------------------------------------------------------------

def flat_views(origins, colours):
    """identity-rotation cameras at `origins` that all see the world origin, images of one colour each, and disparity maps of the
    plane z = 0 (1 / the camera's height)."""
    poses = np.stack([Wn.pose((0., 0., 0.), o) for o in origins])
    images = np.stack([np.broadcast_to(np.asarray(c, np.uint8), (H, W, 3)) for c in colours])
    disp = np.stack([np.full((H, W), 1.0 / o[2], np.float32) for o in origins])
    return poses, images, disp


def test_blend_weights_are_cos2_of_incidence():
    """The point at the origin with normal +z: from (0, 0, 3) cos^2 = 1, from (2, 0, 4) cos^2 = 16 / 20 = 4/5, so the blend of
    the colours A and B is (A + 0.8 B) / 1.8: (90, 0, 255) and (180, 90, 30) give (130, 40, 155) exactly."""
    poses, images, disp = flat_views([(0., 0., 3.), (2., 0., 4.)], [(90, 0, 255), (180, 90, 30)])
    p, nrm = np.zeros((1, 3)), np.array([[0., 0., 2.5]])    # the normal's length does not matter
    rgb, wsum, best, wts = T.bake(p, nrm, images, disp, poses, FOCAL, details=True)
    assert wts[:, 0].tolist() == [1.0, 0.8] and wsum[0] == np.float32(1.8) and best[0] == 0
    assert rgb[0].tolist() == [130, 40, 155]
    assert T.bake(p, nrm, images, disp, poses, FOCAL, mode='best')[0][0].tolist() == [90, 0, 255]
    rgb, _, best = T.bake(p, nrm, images[::-1], disp[::-1], poses[::-1], FOCAL)       # the order of the views
    assert rgb[0].tolist() == [130, 40, 155] and best[0] == 1
    # facing: seen from below the normal points away; cull 'none' takes that view too, with the same weight
    assert T.bake(p, -nrm, images, disp, poses, FOCAL)[2][0] == -1
    assert T.bake(p, -nrm, images, disp, poses, FOCAL, cull='none', details=True)[3][:, 0].tolist() == [1.0, 0.8]


def test_best_ties_go_to_the_lower_index():
    poses, images, disp = flat_views([(2., 0., 4.), (-2., 0., 4.)], [(10, 20, 30), (200, 210, 220)])      # a mirror-symmetric pair
    p, nrm = np.zeros((1, 3)), np.array([[0., 0., 1.]])
    for order in (slice(None), slice(None, None, -1)):
        rgb, wsum, best, wts = T.bake(p, nrm, images[order], disp[order], poses[order], FOCAL, mode='best', details=True)
        assert wts[0, 0] == wts[1, 0] == 0.8 and best[0] == 0
        assert rgb[0].tolist() == images[order][0, 0, 0].tolist()
    assert T.bake(p, nrm, images, disp, poses, FOCAL)[0][0].tolist() == [105, 115, 125]


# ---- 5. the edges of the image ----------------------------------------------------------------------------------------------------

def test_image_borders_near_plane_nan_and_zero_normal():
    """focal 64 and depth 2 make the projections exact: x = 0.96875 lands on u = W - 1 = 63, y = 0.75 on w = 0."""
    focal = 64.0
    images = np.random.RandomState(3).randint(0, 256, (1, H, W, 3)).astype(np.uint8)
    disp = np.full((1, H, W), 0.5, np.float32)
    up = np.float32(np.nextafter(np.float32(0.96875), np.float32(2)))
    pts = np.array([[0.96875, 0.125, -2], [up, 0.125, -2], [0.25, 0.75, -2], [0.25, np.nextafter(np.float32(0.75), np.float32(2)), -2],
                    [-1.0, -0.71875, -2], [0.25, 0.125, -2]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(pts), 1))
    u, w, z = T.project_point(pts.astype(F64), IDENTITY, H, W, focal)
    assert u[0] == W - 1 and u[1] > W - 1 and w[2] == 0 and w[3] < 0 and u[4] == 0 and w[4] == H - 1 and (z == 2).all()
    rgb, wsum, best = T.bake_points(pts, nrm, images, disp, IDENTITY[None], focal)
    assert best.tolist() == [0, -1, 0, -1, 0, 0]
    # on the border the clamp x1 = min(x0 + 1, W - 1) keeps the footprint inside: the colour is that of the border pixels alone
    assert rgb[0].tolist() == np.floor(images[0, 20, 63] + 0.5).astype(int).tolist()         # w = 24 - 64 * .125 / 2 = 20
    assert rgb[2].tolist() == images[0, 0, 40].tolist() and rgb[4].tolist() == images[0, 47, 0].tolist()
    assert (rgb[[1, 3]] == 0).all() and (wsum[[1, 3]] == 0).all()
    # nearer than near; behind the camera; a NaN and an infinite point; a zero, a NaN and an infinite normal
    bad_p = np.array([[0, 0, -0.0005], [0, 0, 2], [np.nan, 0, -2], [0, np.inf, -2]], np.float32)
    r = T.bake_points(bad_p, nrm[:4], images, np.full((1, H, W), 2000.0, np.float32), IDENTITY[None], focal)
    assert (r[2] == -1).all() and (r[1] == 0).all() and (r[0] == 0).all()
    ok_p = np.tile(pts[5:6], (4, 1))
    bad_n = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, 1]], np.float32)
    r = T.bake_points(ok_p, bad_n, images, disp, IDENTITY[None], focal)
    assert r[2].tolist() == [-1, -1, -1, 0]
    # the disparity test: a map that is 0, negative, NaN, infinite or off by more than tol at ONE footprint pixel rejects the view
    for value in (0.0, -0.5, np.nan, np.inf, 0.5 * 1.06, 0.5 * 0.94):
        d = disp.copy()
        d[0, 21, 41] = value                                # pts[5] lands on (40.0, 20.0): footprint x 40, 41 (fx = 0), y 20, 21
        assert T.bake_points(pts[5:6], nrm[:1], images, d, IDENTITY[None], focal)[2][0] == -1, value
    d = disp.copy()
    d[0, 21, 41] = 0.5 * 1.04
    assert T.bake_points(pts[5:6], nrm[:1], images, d, IDENTITY[None], focal)[2][0] == 0
    # no views, no points
    e = T.bake_points(pts, nrm, np.zeros((0, H, W, 3), np.uint8), np.zeros((0, H, W), np.float32), np.zeros((0, 3, 4), np.float32), focal)
    assert (e[2] == -1).all() and (e[0] == 0).all()
    assert T.bake_points(np.zeros((0, 3)), np.zeros((0, 3)), images, disp, IDENTITY[None], focal)[0].shape == (0, 3)


# ---- 6. the OBJ export ------------------------------------------------------------------------------------------------------------

def read_png(path):
    """a minimal decoder of 8-bit RGB PNGs whose rows use filter 0 (what run._write_png writes)."""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, size = 8, b'', None
    while pos < len(raw):
        length, tag = struct.unpack('>I', raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        data = raw[pos + 8:pos + 8 + length]
        assert struct.unpack('>I', raw[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(tag + data) & 0xffffffff
        if tag == b'IHDR':
            w, h, depth, kind = struct.unpack('>IIBB', data[:10])
            assert (depth, kind) == (8, 2)
            size = (h, w)
        elif tag == b'IDAT':
            idat += data
        pos += 12 + length
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + 3 * size[1])
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(size[0], size[1], 3)


def test_save_obj_round_trip(tmp_path):
    n = 3
    v, f, poses, images, disp, _ = occlusion_scene()
    rgb, wsum, _ = T.bake_atlas(v, f, n, images, disp, poses, FOCAL)
    normals = R.vertex_normals(v, f).astype(np.float32)
    shape, uv = mesh.atlas_layout(len(f), n)
    assert shape == rgb.shape
    tex = mesh.Texture(rgb, uv, wsum > 0, n)
    path = str(tmp_path / 'quads.obj')
    files = mesh.save_obj(path, mesh.Mesh(v, f, normals, None), tex)
    assert [os.path.basename(p) for p in files] == ['quads.obj', 'quads.mtl', 'quads.png'] and all(os.path.exists(p) for p in files)
    rows = [line.split() for line in open(path).read().splitlines() if line and not line.startswith('#')]
    by = lambda key: [r[1:] for r in rows if r[0] == key]
    gv, gn, gt = (np.array(by(k), float) for k in ('v', 'vn', 'vt'))
    assert np.array_equal(gv.astype(np.float32), v) and np.array_equal(gn.astype(np.float32), normals)
    assert gt.shape == (3 * len(f), 2) and gt.min() >= 0 and gt.max() <= 1 and np.array_equal(gt.astype(np.float32), uv.reshape(-1, 2))
    gf = np.array([[[int(x) for x in corner.split('/')] for corner in r] for r in by('f')])           # [F, 3 corners, v/t/n]
    assert gf.shape == (len(f), 3, 3) and np.array_equal(gf[..., 0] - 1, f) and np.array_equal(gf[..., 2], gf[..., 0])
    assert np.array_equal(gf[..., 1].reshape(-1), np.arange(1, 3 * len(f) + 1))                     # 1-based, one vt per corner
    assert by('mtllib') == [['quads.mtl']] and by('usemtl') == [['quads']]
    mtl = [line.split() for line in open(files[1]).read().splitlines()]
    assert ['newmtl', 'quads'] in mtl and ['map_Kd', 'quads.png'] in mtl
    assert np.array_equal(read_png(files[2]), rgb)          # PNG row 0 is the texture's row 0
    # the texel a vt names: u Wt, (1 - v) Ht are the continuous coordinates of the corner texel's centre
    face, _, _ = T.owner_map(len(f), n)
    X, Y = np.floor(gt[:, 0] * shape[1]).astype(int), np.floor((1 - gt[:, 1]) * shape[0]).astype(int)
    assert np.array_equal(face[Y, X], np.repeat(np.arange(len(f)), 3))
    plain = mesh.save_obj(str(tmp_path / 'plain.obj'), mesh.Mesh(v, f, normals, None))
    text = open(plain[0]).read()
    assert len(plain) == 1 and 'vt ' not in text and 'mtllib' not in text and 'f 1//1 2//2 3//3' in text


# ---- 7. what a texture carries that vertex colours cannot -------------------------------------------------------------------------

CARRY_CELL, CARRY_TEXELS = 3.0, 8


def coarse_sphere():
    v, f, _ = M.marching_cubes(R.lattice(24, R.sphere_field()), 1.0, R.LO, R.HI)
    res = R.cluster(v, f, None, None, CARRY_CELL * R.step(24), 'mean')
    return res['verts'], res['faces']


def test_texture_carries_what_vertex_colours_cannot():
    """The 24^3 sphere (1,772 faces) clustered in cells of 3 lattice steps (166 faces, 85 vertices), seen by the first camera of
    tests/test_raster.py; the image is a checkerboard of 4-pixel squares (40 / 220) on the pixels the clustered mesh itself
    covers.  (One view: checkerboards drawn in the image planes of two cameras contradict each other on the surface, and a
    blend of them measures that contradiction, not the texture.)  The textured render (8 texels per leg) against the image must
    beat the best the parent commit can express: the same mesh with colours baked at its vertices from the same view,
    interpolated by the rasteriser.  Compared over the pixels covered in both, that is whose winning face has all three vertices
    coloured by the view (247 of the 435 covered pixels; the rim's vertices are seen by no footprint that lies wholly on the
    mesh).  Measured with the numpy restatement: RMS error 26.56 levels with the texture against 106.54 with vertex colours."""
    v, f = coarse_sphere()
    poses = Wn.pose((0., 0., 0.), (0., 0., 3.))[None]
    disp, fmap, _ = N.rasterize(v, f, poses, H, W, FOCAL)
    covered = fmap >= 0
    y, x = np.mgrid[0:H, 0:W]
    board = np.where(((x // 4) + (y // 4)) % 2 == 0, 40, 220).astype(np.uint8)
    images = np.where(covered[..., None], board[None, :, :, None], 0).astype(np.uint8).repeat(3, -1)
    atlas, wsum, _ = T.bake_atlas(v, f, CARRY_TEXELS, images, disp, poses, FOCAL)
    _, fm2, textured = T.render_textured(v, f, atlas, CARRY_TEXELS, poses, H, W, FOCAL)
    normals = R.vertex_normals(v, f).astype(np.float32)
    colours, seen, _ = T.bake_points(v, normals, images, disp, poses, FOCAL)
    _, fm3, vertex = N.rasterize(v, f, poses, H, W, FOCAL, colors=colours)
    assert np.array_equal(fm2, fmap) and np.array_equal(fm3, fmap)
    # covered in both: the pixels whose winning face has all three vertices coloured by some view (elsewhere the vertex render
    # interpolates towards a vertex no view saw; a texel no view saw still counts, against the texture)
    both = covered & (seen > 0)[f[np.where(covered, fmap, 0)]].all(-1)
    assert both.sum() > 0.5 * covered.sum()
    rms = lambda a: float(np.sqrt(np.mean((a[both].astype(F64) - images[both].astype(F64)) ** 2)))
    r_tex, r_vert = rms(textured), rms(vertex)
    print(f'clustered sphere: {len(f)} faces, {len(v)} vertices, {int(both.sum())} of {int(covered.sum())} covered pixels compared; RMS error textured {r_tex:.2f}, '
          f'vertex colours {r_vert:.2f} levels')
    assert r_tex < r_vert
