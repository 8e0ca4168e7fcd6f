"""numpy restatement of the mesh rasteriser (csrc/raster.hip; ops.mesh_rasterize), written from the definition alone -- the role
tests/mesh_ops_numpy.py has for the mesh clean-up.  Everything is fp64 and integers, so the kernels must agree BIT FOR BIT.

The camera (project and its conventions) is tests/camera_numpy.py's with T = fp64; faces are counter-clockwise seen from outside.

Per view, per vertex p (fp32 widened to fp64):
    (u, w, z) = project(pose, p);  d = 1 / z
    X = rint(256 u), Y = rint(256 w)                  8 sub-pixel bits, ties to even, integers from here on
Per face: dropped whole for the view unless every vertex has z >= near and |256 u|, |256 w| <= 2^22 (compared in fp64 before
the conversion; a NaN fails).  THERE IS NO NEAR-PLANE CLIPPING: a face that straddles z = near vanishes.  A2 = (X1 - X0)(Y2 - Y0)
- (Y1 - Y0)(X2 - X0) (x right, y down): A2 = 0 dropped; A2 < 0 is front-facing; cull='back' drops A2 > 0; when A2 < 0 vertices
1 and 2 are swapped (positions, d and colours), so that A2 > 0 from here on.
Coverage of pixel (x, y), sx = 256 x, sy = 256 y: for the edge from vertex i to j opposite k (k = 0: 1 -> 2, k = 1: 2 -> 0,
k = 2: 0 -> 1), E_k = (Xj - Xi)(sy - Yi) - (Yj - Yi)(sx - Xi); covered iff every E_k > 0, or E_k = 0 and, with (ex, ey) =
(Xj - Xi, Yj - Yi), ey < 0 or (ey = 0 and ex > 0) -- the coverage of the sample point (x + eps, y + eps^2), the top-left rule.
Fragment: D = fp32(((E0 d0 + E1 d1) + E2 d2) / A2); skipped unless D is finite and > 0.
Resolution: per pixel the largest key (bits(D) << 32) | (0xFFFFFFFF - face) wins: the nearest fragment, the lower face index on
equal disparity.  disp = D of the winner (0 where none), face = its index (-1 where none), and with colours rgb = floor(c + .5)
clamped to 0..255 of c = ((b0 c0 + b1 c1) + b2 c2) / ((b0 + b1) + b2), b_k = E_k d_k, recomputed for the winner (0 where none).
"""
import numpy as np

import camera_numpy as C

F32, F64, I64 = np.float32, np.float64, np.int64
SUB = 256
BAND = 2.0 ** 22
CULLS = ('none', 'back')


def project(verts, c2w, H, W, focal, near):
    """(X, Y int64 [Nv], d fp64 [Nv], ok bool [Nv]) of one view; X = Y = 0 where not ok."""
    p = np.asarray(verts, F32).astype(F64).reshape(-1, 3)
    u, w, z = C.project(F64, np.asarray(c2w, F32).astype(F64).reshape(3, 4), F64(focal), H, W, p.T)
    with np.errstate(all='ignore'):
        d = 1.0 / z
        su, sw = 256.0 * u, 256.0 * w
        ok = (z >= F64(near)) & (np.abs(su) <= BAND) & (np.abs(sw) <= BAND)
        X = np.where(ok, np.rint(np.where(ok, su, 0.0)), 0.0).astype(I64)
        Y = np.where(ok, np.rint(np.where(ok, sw, 0.0)), 0.0).astype(I64)
    return X, Y, d, ok


def _edges(X, Y, sx, sy):
    """E_k and their ownership for vertex arrays X, Y [..., 3] (already swapped so that A2 > 0) at the sample (sx, sy)."""
    E, own = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        ex, ey = X[..., j] - X[..., i], Y[..., j] - Y[..., i]
        E.append(ex * (sy - Y[..., i]) - ey * (sx - X[..., i]))
        own.append((ey < 0) | ((ey == 0) & (ex > 0)))
    return E, own


def _oriented(X, Y, d, f):
    """The three vertices of faces f [..., 3] with 1 and 2 swapped where A2 < 0: (Xf, Yf, df, A2 > 0 or 0, swapped)."""
    Xf, Yf, df = X[f], Y[f], d[f]
    A2 = (Xf[..., 1] - Xf[..., 0]) * (Yf[..., 2] - Yf[..., 0]) - (Yf[..., 1] - Yf[..., 0]) * (Xf[..., 2] - Xf[..., 0])
    sw = A2 < 0
    order = np.where(sw[..., None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    take = lambda a: np.take_along_axis(a, order, -1)
    return take(Xf), take(Yf), take(df), np.abs(A2), A2, order


def rasterize_view(verts, faces, c2w, H, W, focal, near=1e-3, cull='none', colors=None):
    """-> dict(disp fp32 [H, W], face int32 [H, W], rgb uint8 [H, W, 3] | None, fragments int64 [H, W]: the fragments every
    pixel received, front [F] bool: A2 < 0 among the faces that were not dropped)."""
    assert cull in CULLS
    f = np.asarray(faces, I64).reshape(-1, 3)
    Nv = np.asarray(verts).reshape(-1, 3).shape[0]
    if f.size and (f.min() < 0 or f.max() >= Nv):
        raise ValueError(f'a face index lies outside [0, {Nv})')
    X, Y, d, ok = project(verts, c2w, H, W, focal, near)
    keys = np.zeros((H, W), np.uint64)
    frags = np.zeros((H, W), I64)
    front = np.zeros(len(f), bool)
    if len(f):
        Xf, Yf, df, A2, A2s, _ = _oriented(X, Y, d, f)
        keep = ok[f].all(-1) & (A2s != 0)
        front = keep & (A2s < 0)
        if cull == 'back':
            keep &= A2s < 0
        for n in np.nonzero(keep)[0]:
            x0, x1 = max(0, -((-int(Xf[n].min())) // SUB)), min(W - 1, int(Xf[n].max()) // SUB)
            y0, y1 = max(0, -((-int(Yf[n].min())) // SUB)), min(H - 1, int(Yf[n].max()) // SUB)
            if x0 > x1 or y0 > y1:
                continue
            sy, sx = np.meshgrid(np.arange(y0, y1 + 1, dtype=I64) * SUB, np.arange(x0, x1 + 1, dtype=I64) * SUB, indexing='ij')
            E, own = _edges(Xf[n], Yf[n], sx, sy)
            cov = np.ones(sx.shape, bool)
            for k in range(3):
                cov &= (E[k] > 0) | ((E[k] == 0) & own[k])
            if not cov.any():
                continue
            with np.errstate(all='ignore'):
                D = (((E[0].astype(F64) * df[n, 0] + E[1].astype(F64) * df[n, 1]) + E[2].astype(F64) * df[n, 2])
                     / F64(A2[n])).astype(F32)
            cov &= np.isfinite(D) & (D > 0)
            key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(n))
            box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            keys[box] = np.where(cov, np.maximum(keys[box], key), keys[box])
            frags[box] += cov
    hit = keys != 0
    disp = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    face = np.where(hit, 0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(I64), -1).astype(np.int32)
    rgb = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).reshape(-1, 3).astype(F64)
        rgb = np.zeros((H, W, 3), np.uint8)
        ys, xs = np.nonzero(hit)
        if len(ys):
            fw = f[face[ys, xs]]
            Xf, Yf, df, _, _, order = _oriented(X, Y, d, fw)
            cf = np.take_along_axis(col[fw], order[..., None], 1)                      # [n, 3 vertices, 3 channels]
            E, _ = _edges(Xf, Yf, xs.astype(I64) * SUB, ys.astype(I64) * SUB)
            b = [E[k].astype(F64) * df[:, k] for k in range(3)]
            den = (b[0] + b[1]) + b[2]
            for ch in range(3):
                c = ((b[0] * cf[:, 0, ch] + b[1] * cf[:, 1, ch]) + b[2] * cf[:, 2, ch]) / den
                rgb[ys, xs, ch] = np.clip(np.floor(c + 0.5), 0.0, 255.0).astype(np.uint8)
    return {'disp': disp, 'face': face, 'rgb': rgb, 'fragments': frags, 'front': front}


def rasterize(verts, faces, poses, H, W, focal, near=1e-3, cull='none', colors=None):
    """(disp [V, H, W] fp32, face [V, H, W] int32, rgb [V, H, W, 3] uint8 | None): what ops.mesh_rasterize returns."""
    poses = np.asarray(poses, F32).reshape(-1, 3, 4)
    views = [rasterize_view(verts, faces, P, H, W, focal, near, cull, colors) for P in poses]
    disp = np.stack([v['disp'] for v in views]) if views else np.zeros((0, H, W), F32)
    face = np.stack([v['face'] for v in views]) if views else np.zeros((0, H, W), np.int32)
    rgb = None
    if colors is not None:
        rgb = np.stack([v['rgb'] for v in views]) if views else np.zeros((0, H, W, 3), np.uint8)
    return disp, face, rgb


def keep_faces(verts, faces, keep, normals=None, colors=None):
    """The mesh with only the faces keep [F] bool marks: unreferenced vertices dropped, order preserved, attributes carried."""
    f = np.asarray(faces, I64).reshape(-1, 3)[np.asarray(keep, bool)]
    used = np.zeros(len(verts), bool)
    used[f.reshape(-1)] = True
    new = np.cumsum(used) - 1
    pick = lambda a: None if a is None else np.asarray(a)[used]
    return np.asarray(verts)[used], new[f].astype(np.int32), pick(normals), pick(colors)
