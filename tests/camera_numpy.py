"""The pinhole camera of the view-space kernels restated in numpy (TEST HELPER, not collected): what csrc/camera_device.h
computes, in the precision T (np.float64: the yardstick; np.float32: the fp32 kernels' own arithmetic, operation for operation).

Conventions: a pose is c2w [3, 4] = [R | o]; the camera looks down -z; no half-pixel offset (pixel (x, y) is the sample point
u = x, v = y); the ray parameter is the planar depth t, disparity = 1 / t.
    unproject:  dx = (x - W * .5) / f,  dy = -((y - H * .5) / f),  p_c = (t dx, t dy, -t)
                p_w[c] = ((p_c[0] R[c][0] + p_c[1] R[c][1]) + p_c[2] R[c][2]) + o[c]
    project:    dl = p - o,  q[j] = (R[0][j] dl[0] + R[1][j] dl[1]) + R[2][j] dl[2],  z = -q[2]
                u = (f q[0]) / z + W * .5,  v = -((f q[1]) / z) + H * .5
Poses and focal lengths enter already in T (the callers widen the fp32 values the kernels receive); points and positions are
tuples of three / two arrays of one shape.
"""
import numpy as np


def pose(angles=(0., 0., 0.), origin=(0., 0., 0.), dtype=np.float32):
    """c2w [3, 4]: rotations about x, y, z (radians) composed as Rz Ry Rx in fp64, and the camera centre; rounded to `dtype`."""
    ax, ay, az = angles
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(origin, np.float64)[:, None]], 1).astype(dtype)


def pixel_dir(T, xs, ys, H, W, f):
    """(dx, dy) of the camera-space direction (dx, dy, -1) of the pixels (xs, ys)."""
    half = T(.5)
    return (xs.astype(T) - T(W) * half) / f, -((ys.astype(T) - T(H) * half) / f)


def unproject(T, c2w, H, W, f, xs, ys, t):
    """The world points (three arrays) at planar depth t along the rays of the pixels (xs, ys)."""
    dx, dy = pixel_dir(T, xs, ys, H, W, f)
    pc = (t * dx, t * dy, -t)
    R, o = c2w[:, :3], c2w[:, 3]
    return [((pc[0] * R[c, 0] + pc[1] * R[c, 1]) + pc[2] * R[c, 2]) + o[c] for c in range(3)]


def project(T, c2w, f, H, W, p):
    """(u, v, z): the continuous image positions and the planar depths of the world points p; nothing is tested."""
    R, o = c2w[:, :3], c2w[:, 3]
    half = T(.5)
    with np.errstate(all='ignore'):
        dl = [p[c] - o[c] for c in range(3)]
        q = [(R[0, j] * dl[0] + R[1, j] * dl[1]) + R[2, j] * dl[2] for j in range(3)]
        z = -q[2]
        return (f * q[0]) / z + T(W) * half, -((f * q[1]) / z) + T(H) * half, z


def in_image(z, u, v, H, W):
    """In front of the camera and on the closed pixel lattice [0, W-1] x [0, H-1]; a NaN fails every comparison."""
    with np.errstate(invalid='ignore'):
        return (z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)


def lower_footprint(u, v, H, W):
    """(x0, y0 int64, fx, fy): the 2 x 2 bilinear footprint from its lower corner, x0 = min(floor(u), W - 2), fx = u - x0.  Only
    in_image positions count; the others (a NaN as 0) are clamped into the image so that a caller can still look at the taps."""
    T = u.dtype.type
    with np.errstate(invalid='ignore'):
        x0 = np.clip(np.floor(np.where(np.isfinite(u), u, 0)), 0, W - 2).astype(np.int64)
        y0 = np.clip(np.floor(np.where(np.isfinite(v), v, 0)), 0, H - 2).astype(np.int64)
        return x0, y0, u - x0.astype(T), v - y0.astype(T)


def lower_blend(a, y0, x0, fy, fx):
    """The bilinear value of the image a [H, W] or [H, W, C] on a lower_footprint: each row first, then the two rows."""
    one = fx.dtype.type(1)
    gx, gy = one - fx, one - fy
    if a.ndim == 3:
        fx, fy, gx, gy = fx[:, None], fy[:, None], gx[:, None], gy[:, None]
    top = a[y0, x0] * gx + a[y0, x0 + 1] * fx
    bot = a[y0 + 1, x0] * gx + a[y0 + 1, x0 + 1] * fx
    return top * gy + bot * fy


def project_points(points, c2w, focal, H, W):
    """fp64 (z, u, v) of world points [..., 3] in camera c2w, in matrix form: for the tests' own bookkeeping, not part of the
    definition."""
    c2w = np.asarray(c2w, np.float64)
    q = (points - c2w[:, 3]) @ c2w[:, :3]
    z = -q[..., 2]
    return z, focal * q[..., 0] / z + W * .5, -(focal * q[..., 1] / z) + H * .5
