"""numpy restatement of the mesh texturing (csrc/texture.hip; ops.mesh_bake_points / mesh_bake_atlas / mesh_texture_resolve),
written from the definition alone -- the role tests/raster_numpy.py has for the rasteriser.  Everything is fp64 + - * /, floor
and integers, so the kernels must agree BIT FOR BIT.

ATLAS LAYOUT, a pure integer function of (F, n); n = texels along a face's leg, 1..32.  S = n + 3; faces 2k and 2k + 1 share block
k; B = ceil(F / 2) blocks row-major, Bx = the smallest integer with Bx Bx >= B per row, By = ceil(B / Bx); texture [By S, Bx S, 3]
bytes, a side at most 16,384.  Texel (X, Y): bx = X div S, by = Y div S, k = by Bx + bx, (i, j) = (X - bx S, Y - by S); i + j <=
S - 1: owner 2k with (i, j), otherwise owner 2k + 1 with (S - 1 - i, S - 1 - j); an owner >= F is none (-1) and the texel holds 0.
Sample point of an owned texel:  i + j < n: l1 = i / n, l2 = j / n, l0 = (1 - l1) - l2;  i + j >= n: m = min(max(i - j + n, 0),
2 n), l1 = m / (2 n), l2 = (2 n - m) / (2 n), l0 = 0 (the texel projected onto the hypotenuse and clamped to its end points).
p = (l0 p0 + l1 p1) + l2 p2 in fp64; nrm = (p1 - p0) x (p2 - p0) in fp64.  UV corners in continuous texel coordinates (centres at
integer + 1/2): lower half (bx S + 1/2 + n l1, by S + 1/2 + n l2), upper half ((bx + 1) S - 1/2 - n l1, (by + 1) S - 1/2 - n l2).

BAKE of a point p with normal nrm, views in ascending order.  View v contributes iff all of: (u, w, z) = the projection of
tests/raster_numpy.py with z >= near; 0 <= u <= W - 1, 0 <= w <= H - 1; l = o - p, c = (nrm0 l0 + nrm1 l1) + nrm2 l2 with c > 0
(cull 'back') or c != 0 ('none'); nn = (nrm0^2 + nrm1^2) + nrm2^2 > 0, ll likewise, wgt = (c c) / (nn ll) finite and > 0;
x0 = floor(u), x1 = min(x0 + 1, W - 1), fx = u - x0 (y likewise); at all four footprint pixels the disparity D of the rasterised
mesh is finite, > 0, |D z - 1| <= tol, and the mask (if given) True.  A NaN anywhere fails.  Colour per channel: top = c00 +
fx (c10 - c00), bot = c01 + fx (c11 - c01), col = top + fy (bot - top).  'blend': floor((sum wgt col) / (sum wgt) + 1/2), sums in
view order; 'best': floor(col + 1/2) of the view of largest wgt, the lower index on a tie; clamped to 0..255.  wsum = fp32(sum
wgt), best = the view of largest weight or -1; rgb 0 where no view contributes.

TEXTURED RESOLVE of a face map: for face >= 0 the winner's set-up and b_k = E_k d_k, den = (b0 + b1) + b2 as the rasteriser's
colour resolve; la = b1 / den, lb = b2 / den of the set-up's vertices 1 and 2, (l1, l2) = swapped ? (lb, la) : (la, lb); lower half
sx = bx S + n l1, sy = by S + n l2, upper half sx = (bx S + S - 1) - n l1, sy = (by S + S - 1) - n l2; with 0 <= sx <= Wt - 1,
0 <= sy <= Ht - 1 the bilinear value of the atlas there (x1 = min(x0 + 1, Wt - 1)), floor(c + 1/2) clamped; else 0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_numpy as C                                 # noqa: E402
import raster_numpy as N                                 # noqa: E402

F32, F64, I64 = np.float32, np.float64, np.int64
MAX_SIDE = 16384
CULLS = ('none', 'back')
MODES = ('blend', 'best')


def layout(F, n):
    """dict(n, S, Bx, By, Wt, Ht); ValueError for n outside 1..32 or a side over 16,384."""
    F, n = int(F), int(n)
    if F < 0 or not 1 <= n <= 32:
        raise ValueError(f'atlas: F >= 0 and texels in 1..32 expected, got {F}, {n}')
    S = n + 3
    B = (F + 1) // 2
    Bx = 0
    while Bx * Bx < B:
        Bx += 1
    By = -(-B // Bx) if Bx else 0
    if Bx * S > MAX_SIDE or By * S > MAX_SIDE:
        raise ValueError(f'atlas: {F} faces at {n} texels need a texture of {By * S} x {Bx * S}, over {MAX_SIDE}')
    return {'n': n, 'S': S, 'Bx': Bx, 'By': By, 'Wt': Bx * S, 'Ht': By * S}


def owner_map(F, n):
    """(face [Ht, Wt] int64, -1 = none; i, j [Ht, Wt] int64: the texel's coordinates in its owner's half)."""
    L = layout(F, n)
    S = L['S']
    Y, X = np.mgrid[0:L['Ht'], 0:L['Wt']].astype(I64)
    bx, by = X // S, Y // S
    i, j = X - bx * S, Y - by * S
    upper = i + j > S - 1
    face = 2 * (by * L['Bx'] + bx) + upper
    i, j = np.where(upper, S - 1 - i, i), np.where(upper, S - 1 - j, j)
    return np.where(face < F, face, -1), i, j


def lambdas(n, i, j):
    """fp64 (l0, l1, l2) of the texels (i, j) of a half."""
    i, j = np.asarray(i, I64), np.asarray(j, I64)
    inner = i + j < n
    m = np.clip(i - j + n, 0, 2 * n)
    l1 = np.where(inner, i.astype(F64) / F64(n), m.astype(F64) / F64(2 * n))
    l2 = np.where(inner, j.astype(F64) / F64(n), (2 * n - m).astype(F64) / F64(2 * n))
    l0 = np.where(inner, (1.0 - l1) - l2, 0.0)
    return l0, l1, l2


def atlas_uv(F, n):
    """((Ht, Wt, 3), uv [F, 3, 2] fp32 in OBJ convention: u = x / Wt, v = 1 - y / Ht of the corners' continuous coordinates)."""
    L = layout(F, n)
    S = L['S']
    f = np.arange(F, dtype=I64)
    k = f // 2
    by, bx = (k // L['Bx'], k % L['Bx']) if F else (k, k)
    upper = (f % 2 == 1)[:, None]
    a = np.array([0.0, n, 0.0])[None]                       # n l1 of the three corners
    b = np.array([0.0, 0.0, n])[None]
    x = np.where(upper, ((bx + 1) * S)[:, None] - 0.5 - a, (bx * S)[:, None] + 0.5 + a)
    y = np.where(upper, ((by + 1) * S)[:, None] - 0.5 - b, (by * S)[:, None] + 0.5 + b)
    uv = np.stack([x / F64(max(L['Wt'], 1)), 1.0 - y / F64(max(L['Ht'], 1))], -1).astype(F32)
    return (L['Ht'], L['Wt'], 3), uv


def atlas_points(verts, faces, n):
    """(face [Ht, Wt], p [Ht, Wt, 3] fp64, nrm [Ht, Wt, 3] fp64, (l0, l1, l2)); p = nrm = 0 where face = -1."""
    v = np.asarray(verts, F32).astype(F64).reshape(-1, 3)
    f = np.asarray(faces, I64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f'a face index lies outside [0, {len(v)})')
    face, i, j = owner_map(len(f), n)
    l0, l1, l2 = lambdas(n, i, j)
    own = face >= 0
    if not len(f):
        z = np.zeros(face.shape + (3,), F64)
        return face, z, z.copy(), (l0, l1, l2)
    fv = v[f[np.where(own, face, 0)]]                        # [Ht, Wt, 3 vertices, 3]
    p0, p1, p2 = fv[..., 0, :], fv[..., 1, :], fv[..., 2, :]
    with np.errstate(all='ignore'):
        p = (l0[..., None] * p0 + l1[..., None] * p1) + l2[..., None] * p2
        e1, e2 = p1 - p0, p2 - p0
        nrm = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                        e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
    return face, np.where(own[..., None], p, 0.0), np.where(own[..., None], nrm, 0.0), (l0, l1, l2)


def project_point(p, c2w, H, W, focal):
    """(u, w, z) fp64 [N] of fp64 points p [N, 3]: the projection of raster_numpy.project, nothing tested."""
    return C.project(F64, np.asarray(c2w, F32).astype(F64).reshape(3, 4), F64(focal), H, W, p.T)


def _bilinear(c00, c10, c01, c11, fx, fy):
    top = c00 + fx * (c10 - c00)
    bot = c01 + fx * (c11 - c01)
    return top + fy * (bot - top)


def _to_byte(c):
    return np.clip(np.floor(c + 0.5), 0.0, 255.0).astype(np.uint8)


def bake(p, nrm, images, disp, poses, focal, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None, details=False):
    """fp64 points p [N, 3] and normals nrm [N, 3] -> (rgb uint8 [N, 3], wsum fp32 [N], best int32 [N]); details=True appends
    the weights [V, N] fp64 (0 where the view does not contribute)."""
    assert cull in CULLS and mode in MODES
    p, nrm = np.asarray(p, F64).reshape(-1, 3), np.asarray(nrm, F64).reshape(-1, 3)
    images = np.asarray(images, np.uint8)
    disp = np.asarray(disp, F32)
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    V = poses.shape[0]
    H, W = (images.shape[1], images.shape[2]) if V else (1, 1)
    Np = p.shape[0]
    near, tol = F64(near), F64(tol)
    sw, sc = np.zeros(Np, F64), np.zeros((Np, 3), F64)
    bw, bc, bi = np.zeros(Np, F64), np.zeros((Np, 3), F64), np.full(Np, -1, np.int32)
    weights = np.zeros((V, Np), F64)
    with np.errstate(all='ignore'):
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        for v in range(V):
            P = poses[v].astype(F64)
            u, w, z = project_point(p, poses[v], H, W, focal)
            ok = (z >= near) & (u >= 0.0) & (u <= F64(W - 1)) & (w >= 0.0) & (w <= F64(H - 1))
            l = [P[a, 3] - p[:, a] for a in range(3)]
            c = (nrm[:, 0] * l[0] + nrm[:, 1] * l[1]) + nrm[:, 2] * l[2]
            ok &= (c > 0.0) if cull == 'back' else ((c > 0.0) | (c < 0.0))
            ll = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]
            wgt = (c * c) / (nn * ll)
            ok &= (nn > 0.0) & (wgt > 0.0) & (wgt <= np.finfo(F64).max)
            us, ws = np.where(ok, u, 0.0), np.where(ok, w, 0.0)
            x0, y0 = np.floor(us).astype(I64), np.floor(ws).astype(I64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            fx, fy = us - x0.astype(F64), ws - y0.astype(F64)
            for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
                D = disp[v, yy, xx].astype(F64)
                ok &= (D > 0.0) & (D <= np.finfo(F64).max) & (np.abs(D * z - 1.0) <= tol)
                if masks is not None:
                    ok &= np.asarray(masks)[v, yy, xx] != 0
            im = images[v].astype(F64)
            col = _bilinear(im[y0, x0], im[y0, x1], im[y1, x0], im[y1, x1], fx[:, None], fy[:, None])      # [N, 3]
            wgt = np.where(ok, wgt, 0.0)
            weights[v] = wgt
            sw = np.where(ok, sw + wgt, sw)
            sc = np.where(ok[:, None], sc + wgt[:, None] * col, sc)
            better = ok & (wgt > bw)
            bw = np.where(better, wgt, bw)
            bc = np.where(better[:, None], col, bc)
            bi = np.where(better, np.int32(v), bi).astype(np.int32)
        seen = bi >= 0
        value = bc if mode == 'best' else sc / np.where(seen, sw, 1.0)[:, None]
        rgb = np.where(seen[:, None], _to_byte(np.where(seen[:, None], value, 0.0)), 0).astype(np.uint8)
    out = (rgb, sw.astype(F32), bi)
    return out + (weights,) if details else out


def bake_points(points, normals, images, disp, poses, focal, **kw):
    """What ops.mesh_bake_points returns for fp32 points and normals [N, 3]."""
    return bake(np.asarray(points, F32).astype(F64), np.asarray(normals, F32).astype(F64), images, disp, poses, focal, **kw)


def bake_atlas(verts, faces, n, images, disp, poses, focal, **kw):
    """What ops.mesh_bake_atlas returns: (rgb [Ht, Wt, 3], wsum [Ht, Wt], best [Ht, Wt]); with details=True also the weights
    [V, Ht, Wt]."""
    face, p, nrm, _ = atlas_points(verts, faces, n)
    out = bake(p.reshape(-1, 3), nrm.reshape(-1, 3), images, disp, poses, focal, **kw)
    own = face >= 0
    shape = face.shape
    rgb = np.where(own[..., None], out[0].reshape(shape + (3,)), 0).astype(np.uint8)
    res = (rgb, np.where(own, out[1].reshape(shape), F32(0)).astype(F32), np.where(own, out[2].reshape(shape), -1).astype(np.int32))
    if len(out) == 4:
        res += (np.where(own[None], out[3].reshape((-1,) + shape), 0.0),)
    return res


def texture_resolve(face_map, verts, faces, atlas, n, poses, H, W, focal, near=1e-3):
    """rgb [V, H, W, 3] uint8 of the textured mesh for the face maps [V, H, W] of raster_numpy.rasterize."""
    f = np.asarray(faces, I64).reshape(-1, 3)
    Nv = np.asarray(verts).reshape(-1, 3).shape[0]
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    atlas = np.asarray(atlas, np.uint8).astype(F64)
    L = layout(len(f), n)
    S, Wt, Ht = L['S'], L['Wt'], L['Ht']
    face_map = np.asarray(face_map)
    out = np.zeros(face_map.shape + (3,), np.uint8)
    for v in range(poses.shape[0]):
        fm = face_map[v]
        ys, xs = np.nonzero((fm >= 0) & (fm < len(f)))
        if not len(ys):
            continue
        fi = fm[ys, xs].astype(I64)
        fw = f[fi]
        inside = ((fw >= 0) & (fw < Nv)).all(-1)
        X, Y, d, ok = N.project(verts, poses[v], H, W, focal, near)
        fws = np.where(inside[:, None], fw, 0)
        Xf, Yf, df, A2, A2s, order = N._oriented(X, Y, d, fws)
        good = inside & ok[fws].all(-1) & (A2s != 0)
        swapped = A2s < 0
        E, _ = N._edges(Xf, Yf, xs.astype(I64) * N.SUB, ys.astype(I64) * N.SUB)
        with np.errstate(all='ignore'):
            b = [E[k].astype(F64) * df[:, k] for k in range(3)]
            den = (b[0] + b[1]) + b[2]
            la, lb = b[1] / den, b[2] / den
            l1, l2 = np.where(swapped, lb, la), np.where(swapped, la, lb)
            k = fi >> 1
            by, bx = k // L['Bx'], k % L['Bx']
            upper = (fi & 1) == 1
            dn = F64(n)
            sx = np.where(upper, (bx * S + S - 1).astype(F64) - dn * l1, (bx * S).astype(F64) + dn * l1)
            sy = np.where(upper, (by * S + S - 1).astype(F64) - dn * l2, (by * S).astype(F64) + dn * l2)
            good &= (sx >= 0.0) & (sx <= F64(Wt - 1)) & (sy >= 0.0) & (sy <= F64(Ht - 1))
            sx, sy = np.where(good, sx, 0.0), np.where(good, sy, 0.0)
            x0, y0 = np.floor(sx).astype(I64), np.floor(sy).astype(I64)
            x1, y1 = np.minimum(x0 + 1, Wt - 1), np.minimum(y0 + 1, Ht - 1)
            fx, fy = (sx - x0.astype(F64))[:, None], (sy - y0.astype(F64))[:, None]
            c = _bilinear(atlas[y0, x0], atlas[y0, x1], atlas[y1, x0], atlas[y1, x1], fx, fy)
        out[v, ys, xs] = np.where(good[:, None], _to_byte(c), 0)
    return out


def render_textured(verts, faces, atlas, n, poses, H, W, focal, near=1e-3, cull='none'):
    """(disp, face, rgb) of the textured mesh in the cameras poses: what mesh.render_textured returns."""
    disp, face, _ = N.rasterize(verts, faces, poses, H, W, focal, near, cull)
    return disp, face, texture_resolve(face, verts, faces, atlas, n, poses, H, W, focal, near)


def bake_texture(verts, faces, n, images, poses, H, W, focal, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None):
    """(rgb, wsum, best) of mesh.bake_texture without a field: the mesh rasterised (cull off) for the disparities, then baked."""
    disp = N.rasterize(verts, faces, poses, H, W, focal, near, 'none')[0]
    return bake_atlas(verts, faces, n, images, disp, poses, focal, near=near, tol=tol, cull=cull, mode=mode, masks=masks)
