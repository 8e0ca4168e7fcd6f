"""Restatement of csrc/harmonic.hip in numpy / scipy.sparse: the harmonic fill's linear system with an fp64 direct solve, an
fp32 conjugate-gradient run of the same recipe as the kernels (its error against the direct solve is the yardstick of the
GPU tests), the 2D mask dilation and the ring-mean baseline.

For one image v [H, W] (fp32) and mask m [H, W] (bool):
  U = m or {p : v_p not finite};  K the rest;  N(p) = the 4-neighbours of p inside the image, deg(p) = |N(p)| (a mirror
  boundary at the image border);  for p in U:  deg(p) u_p - sum_{q in N(p) and U} u_q = sum_{q in N(p) and K} v_q;
  output = v bit for bit on K, u on U.  U empty: v.  U = everything: v, `singular`.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl


def unknown_set(v, m):
    return np.asarray(m, bool) | ~np.isfinite(v)


def system(v, m):
    """(A csr fp64 [n, n], b fp64 [n], deg fp64 [n], U bool [H, W], b32 fp32 [n]); the unknowns are numbered in raster order.
    b32 is the right-hand side as the kernels form it: fp32 additions in the order up, left, right, down."""
    v = np.asarray(v, np.float32)
    U = unknown_set(v, m)
    H, W = U.shape
    idx = -np.ones((H, W), np.int64)
    n = int(U.sum())
    idx[U] = np.arange(n)
    ys, xs = np.nonzero(U)
    deg = np.zeros(n)
    b, b32 = np.zeros(n), np.zeros(n, np.float32)
    rows, cols = [], []
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):                 # up, left, right, down: the kernels' order
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        deg += ok
        yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
        unk = ok & U[yc, xc]
        known = ok & ~U[yc, xc]
        b[known] += v[yc, xc][known].astype(np.float64)
        b32[known] = (b32[known] + v[yc, xc][known]).astype(np.float32)
        rows.append(np.nonzero(unk)[0])
        cols.append(idx[yc, xc][unk])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.coo_matrix((-np.ones(len(rows)), (rows, cols)), shape=(n, n)) + sp.diags(deg)
    return A.tocsr(), b, deg, U, b32


def solve(v, m):
    """(filled fp64 [H, W], singular): the fp64 direct solve.  Known pixels hold v exactly (fp32 values in fp64)."""
    v = np.asarray(v, np.float32)
    A, b, _, U, _ = system(v, m)
    out = v.astype(np.float64)
    if U.all():
        return out, True
    if U.any():
        out[U] = spl.spsolve(A.tocsc(), b) if A.shape[0] > 1 else b / A[0, 0]
    return out, False


def solve_dense(v, m):
    """The same through numpy.linalg.solve (small cases only)."""
    v = np.asarray(v, np.float32)
    A, b, _, U, _ = system(v, m)
    out = v.astype(np.float64)
    if U.any() and not U.all():
        out[U] = np.linalg.solve(A.toarray(), b)
    return out


def cg32(v, m, eps=1e-7, max_iters=None):
    """(filled fp32 [H, W], iterations, converged): Jacobi-preconditioned conjugate gradients in fp32 from a zero start,
    stopped when r.z <= eps^2 r0.z0 on the recursively updated residual -- the kernels' recipe in numpy's summation order."""
    v = np.asarray(v, np.float32)
    A, _, deg, U, b = system(v, m)
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


def dilate(m, rounds):
    """`rounds` rounds of: set iff any pixel at Chebyshev distance <= 1 is set, clipped at the border.  m [..., H, W] bool."""
    m = np.asarray(m, bool)
    for _ in range(rounds):
        p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)])
        H, W = m.shape[-2:]
        out = np.zeros_like(m)
        for dy in range(3):
            for dx in range(3):
                out |= p[..., dy:dy + H, dx:dx + W]
        m = out
    return m


def ring_mean_fill(v, m):
    """Baseline: every unknown pixel gets the mean of the known pixels at Chebyshev distance 1 of the unknown set."""
    v = np.asarray(v, np.float32)
    U = unknown_set(v, m)
    ring = dilate(U, 1) & ~U
    out = v.astype(np.float64)
    if ring.any():
        out[U] = v[ring].astype(np.float64).mean()
    return out
