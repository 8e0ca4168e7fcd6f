"""The definition of cross-view depth consistency, restated in numpy: what csrc/depth_consistency.hip computes, in fp64 on the
fp32 inputs, with the expressions and the association of tests/warp_numpy.py::warp (dtype=np.float64).

A target is a pixel (y, x) of view n with a finite disparity d > 0:
    t = 1 / d,  dx = (x - W * .5) / f,  dy = -((y - H * .5) / f),  p_c = (t dx, t dy, -t)
    p_w[c] = ((p_c[0] R[c][0] + p_c[1] R[c][1]) + p_c[2] R[c][2]) + o[c]
  for every view s != n:
    dl = p_w - o_s,  q[j] = (R_s[0][j] dl[0] + R_s[1][j] dl[1]) + R_s[2][j] dl[2],  t_s = -q[2]
    u = (f q[0]) / t_s + W * .5,  v = -((f q[1]) / t_s) + H * .5
    in range: t_s > 0, 0 <= u <= W - 1, 0 <= v <= H - 1          (a NaN fails every comparison)
    x0 = min(floor(u), W - 2), y0 = min(floor(v), H - 2), fx = u - x0, fy = v - y0
    valid: all four taps of view s's disparity finite and > 0
    d_s = the bilinear value (each row first, then the two rows),  resid = t_s d_s - 1
    agree[n, y, x]    counts the views in range, valid, with |resid| <= tol
    violated[n, y, x] counts the views in range, valid, with resid < -tol     (s sees a farther surface through the point)
    resid > tol: occluded in s, nothing counted
A pixel that is not a target gets 0 / 0.  focal and tol enter as the fp32 values the kernel receives.
"""
import numpy as np

import warp_numpy as wn


def consistency(disp, poses, focal, tol=0.05, masks=None):
    """(agree, violated) int32 [V, H, W]; masks False = the pixel is zeroed first (neither target nor witness)."""
    T = np.float64
    d32 = np.asarray(disp, np.float32)
    if masks is not None:
        d32 = np.where(np.asarray(masks) != 0, d32, np.float32(0))
    V, H, W = d32.shape
    assert H >= 2 and W >= 2
    pose = np.asarray(poses, np.float32).astype(T).reshape(V, 3, 4)
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(d32) & (d32 > 0)
    d = d32.astype(T)
    f, tol = T(np.float32(focal)), T(np.float32(tol))
    one, half = T(1), T(.5)
    agree, violated = np.zeros((V, H, W), np.int32), np.zeros((V, H, W), np.int32)
    for n in range(V):
        ys, xs = np.nonzero(usable[n])
        t = one / d[n, ys, xs]
        dx = (xs.astype(T) - T(W) * half) / f
        dy = -((ys.astype(T) - T(H) * half) / f)
        pc = (t * dx, t * dy, -t)
        R, o = pose[n, :, :3], pose[n, :, 3]
        pw = [((pc[0] * R[c, 0] + pc[1] * R[c, 1]) + pc[2] * R[c, 2]) + o[c] for c in range(3)]
        na, nv = np.zeros(len(ys), np.int32), np.zeros(len(ys), np.int32)
        for s in range(V):
            if s == n:
                continue
            Rs, os_ = pose[s, :, :3], pose[s, :, 3]
            dl = [pw[c] - os_[c] for c in range(3)]
            q = [(Rs[0, j] * dl[0] + Rs[1, j] * dl[1]) + Rs[2, j] * dl[2] for j in range(3)]
            ts = -q[2]
            with np.errstate(all='ignore'):
                u = (f * q[0]) / ts + T(W) * half
                v = -((f * q[1]) / ts) + T(H) * half
                inr = (ts > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                uc, vc = np.where(inr, u, 0), np.where(inr, v, 0)
                x0 = np.minimum(np.floor(uc), W - 2).astype(np.int64)
                y0 = np.minimum(np.floor(vc), H - 2).astype(np.int64)
                valid = usable[s][y0, x0] & usable[s][y0, x0 + 1] & usable[s][y0 + 1, x0] & usable[s][y0 + 1, x0 + 1]
                fx, fy = u - x0.astype(T), v - y0.astype(T)
                ds = wn._bilinear(d[s], y0, x0, fy, fx, one)
                res = ts * ds - one
                ok = inr & valid
                na += ok & (np.abs(res) <= tol)
                nv += ok & (res < -tol)
        agree[n, ys, xs], violated[n, ys, xs] = na, nv
    return agree, violated


# ---- cases shared by tests/test_depth_consistency_cpu.py and tests/test_depth_consistency.py ---------------------------------------

def trial_scene3():
    """warp_numpy.trial_scene() with a third camera: the wall and the box face at 48 x 64, f = 60, analytic disparities rounded
    to fp32.  dict(H, W, focal, poses [3, 3, 4], disp [3, H, W], points [3, H, W, 3] fp64: the world point of every pixel)."""
    c = wn.trial_scene()
    H, W, f = c['H'], c['W'], c['focal']
    third = wn.pose((-0.02, 0.01, -0.01), (0.02, -0.22, 0.03))
    poses = np.stack([c['tgt_pose'][0], c['src_pose'][0], third]).astype(np.float32)
    disp, pts = [], []
    for p in poses:
        d, w = wn.box_scene_disparity(p, H, W, f, **wn.TRIAL_BOX)
        disp.append(d.astype(np.float32))
        pts.append(w)
    return dict(H=H, W=W, focal=f, poses=poses, disp=np.stack(disp), points=np.stack(pts))


FLOATER = (slice(20, 26), slice(8, 14))              # a 6 x 6 patch of view 0, on the wall beside the box


def with_floater(case, factor=1.5):
    """A copy of `case` whose view 0 has the disparity of the FLOATER patch multiplied by `factor`: a blob hanging in free
    space at 1 / factor of the wall's depth."""
    out = dict(case)
    d = case['disp'].copy()
    d[0][FLOATER] *= np.float32(factor)
    out['disp'] = d
    return out


def homography_case3():
    """warp_numpy.homography_case() (33 x 47, one tilted plane) with a third camera; every pixel of every view is on the plane."""
    c = wn.homography_case()
    H, W, f = c['H'], c['W'], c['focal']
    third = wn.pose((0.02, -0.02, 0.04), (0.0, 0.12, -0.05))
    poses = np.stack([c['tgt_pose'][0], c['src_pose'][0], third]).astype(np.float32)
    nrm, off = (0.15, -0.1, 1.0), -3.0
    disp = np.stack([wn.plane_disparity(p, H, W, f, nrm, off).astype(np.float32) for p in poses])
    return dict(H=H, W=W, focal=f, poses=poses, disp=disp)


def project(points, c2w, focal, H, W):
    """fp64 (t_s, u, v) of world points [..., 3] in camera c2w: for the tests' own bookkeeping, not part of the definition."""
    c2w = np.asarray(c2w, np.float64)
    q = (points - c2w[:, 3]) @ c2w[:, :3]
    ts = -q[..., 2]
    return ts, focal * q[..., 0] / ts + W * .5, -(focal * q[..., 1] / ts) + H * .5
