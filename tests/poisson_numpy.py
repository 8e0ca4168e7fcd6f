"""Restatement of the guided (Poisson) variant of csrc/harmonic.hip in numpy / scipy.sparse, on top of tests/harmonic_numpy.py's
`system`: the guided right-hand side in fp64 and in the kernels' fp32 order, the fp64 direct solve, and an fp32
conjugate-gradient run of the kernels' recipe (its error against the direct solve is the yardstick of the GPU tests).

For one image v [H, W] (fp32), mask m [H, W] (bool), guide g [H, W] (fp32) and labels l [H, W] (int32):
  U, K, N(p), deg(p) are harmonic_numpy's (U = m or {v not finite});
  an edge (p, q), q in N(p), is GUIDED iff l_p >= 0, l_q == l_p, and g_p, g_q are both finite;
  for p in U:  deg(p) u_p - sum_{q in N(p) and U} u_q = b_p,  b_p = s_p + t_p,
    s_p = sum_{q in N(p) and K} v_q                   (harmonic_numpy's right-hand side),
    t_p = sum_{q in N(p), (p, q) guided} (g_p - g_q)   (fp32 subtraction, then fp32 addition; up, left, right, down; from 0.f);
  output = v bit for bit on K, u on U.  U empty: v.  U = everything: v, `singular`.
"""
import numpy as np
import scipy.sparse.linalg as spl

import harmonic_numpy as R


def guidance(U, g, l):
    """(t fp64 [n], t32 fp32 [n]) over the unknowns in raster order: the sum of g_p - g_q over the guided edges of p; t32 as the
    kernel forms it."""
    g = np.asarray(g, np.float32)
    l = np.asarray(l, np.int32)
    H, W = U.shape
    ys, xs = np.nonzero(U)
    gp, lp = g[ys, xs], l[ys, xs]
    t, t32 = np.zeros(len(ys)), np.zeros(len(ys), np.float32)
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):                 # up, left, right, down: the kernels' order
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
        gq = g[yc, xc]
        guided = ok & (lp >= 0) & (l[yc, xc] == lp) & np.isfinite(gp) & np.isfinite(gq)
        with np.errstate(invalid='ignore', over='ignore'):
            d32 = (gp - gq).astype(np.float32)                        # fp32 - fp32 in fp32
            d64 = gp.astype(np.float64) - gq.astype(np.float64)
        t[guided] += d64[guided]
        t32[guided] = (t32[guided] + d32[guided]).astype(np.float32)
    return t, t32


def system(v, m, g, l):
    """(A csr fp64 [n, n], b fp64 [n], deg fp64 [n], U bool [H, W], b32 fp32 [n]): harmonic_numpy.system with the guided
    right-hand side; b32 = fp32(s32 + t32), s32 harmonic_numpy's b32."""
    A, s, deg, U, s32 = R.system(v, m)
    t, t32 = guidance(U, g, l)
    return A, s + t, deg, U, (s32 + t32).astype(np.float32)


def solve(v, m, g, l):
    """(filled fp64 [H, W], singular): the fp64 direct solve."""
    v = np.asarray(v, np.float32)
    A, b, _, U, _ = system(v, m, g, l)
    out = v.astype(np.float64)
    if U.all():
        return out, True
    if U.any():
        out[U] = spl.spsolve(A.tocsc(), b) if A.shape[0] > 1 else b / A[0, 0]
    return out, False


def cg32(v, m, g, l, eps=1e-7, max_iters=None):
    """(filled fp32 [H, W], iterations, converged): harmonic_numpy.cg32's loop on the guided b32."""
    v = np.asarray(v, np.float32)
    A, _, deg, U, b = system(v, m, g, l)
    out = v.copy()
    H, W = U.shape
    max_iters = 8 * max(H, W) if max_iters is None else max_iters
    if U.all() or not U.any():
        return out, 0, not U.all()
    f = np.float32
    A, deg = A.astype(f), deg.astype(f)
    x = np.zeros_like(b)
    r = b.copy()
    z = r / deg
    p = z.copy()
    rz = f(np.dot(r, z))
    thr = f(eps) * f(eps) * rz
    it = 0
    while it < max_iters and rz > thr:
        Ap = A @ p
        alpha = rz / f(np.dot(p, Ap))
        x = x + alpha * p
        r = r - alpha * Ap
        z = r / deg
        rz_new = f(np.dot(r, z))
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    out[U] = x
    return out, it, bool(rz <= thr)


def boundary_step(x, mask):
    """Mean |x_p - x_q| over the mask's boundary edges (p in the mask, q a 4-neighbour outside it); x [H, W] or [H, W, C]
    (the mean runs over the channels too).  None without such an edge."""
    x = np.asarray(x, np.float64)
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    total, count = 0.0, 0
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        ys, xs = np.nonzero(mask)
        y, x2 = ys + dy, xs + dx
        ok = (y >= 0) & (y < H) & (x2 >= 0) & (x2 < W)
        ys, xs, y, x2 = ys[ok], xs[ok], y[ok], x2[ok]
        out = ~mask[y, x2]
        d = np.abs(x[ys[out], xs[out]] - x[y[out], x2[out]])
        total += float(d.sum())
        count += d.size
    return total / count if count else None
