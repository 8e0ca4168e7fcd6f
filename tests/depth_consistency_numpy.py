"""The definition of cross-view depth consistency, restated in numpy: what csrc/depth_consistency.hip computes, in fp64 on the
fp32 inputs.  The camera (unproject, project, in_image, lower_footprint, lower_blend) is tests/camera_numpy.py's with T = fp64.

A target is a pixel (y, x) of view n with a finite disparity d > 0:
    p_w = unproject(pose_n, x, y, t = 1 / d)
  for every view s != n:
    (u, v, t_s) = project(pose_s, p_w);  in range: in_image(t_s, u, v)
    valid: all four taps of view s's disparity on the lower_footprint of (u, v) finite and > 0
    d_s = lower_blend of the taps,  resid = t_s d_s - 1
    agree[n, y, x]    counts the views in range, valid, with |resid| <= tol
    violated[n, y, x] counts the views in range, valid, with resid < -tol     (s sees a farther surface through the point)
    resid > tol: occluded in s, nothing counted
A pixel that is not a target gets 0 / 0.  focal and tol enter as the fp32 values the kernel receives.
"""
import numpy as np

import camera_numpy as C
import warp_numpy as wn
from camera_numpy import project_points as project      # noqa: F401  (the tests' fp64 bookkeeping helper)


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
    one = T(1)
    agree, violated = np.zeros((V, H, W), np.int32), np.zeros((V, H, W), np.int32)
    for n in range(V):
        ys, xs = np.nonzero(usable[n])
        pw = C.unproject(T, pose[n], H, W, f, xs, ys, one / d[n, ys, xs])
        na, nv = np.zeros(len(ys), np.int32), np.zeros(len(ys), np.int32)
        for s in range(V):
            if s == n:
                continue
            u, v, ts = C.project(T, pose[s], f, H, W, pw)
            with np.errstate(all='ignore'):
                inr = C.in_image(ts, u, v, H, W)
                x0, y0, fx, fy = C.lower_footprint(u, v, H, W)
                valid = usable[s][y0, x0] & usable[s][y0, x0 + 1] & usable[s][y0 + 1, x0] & usable[s][y0 + 1, x0 + 1]
                ds = C.lower_blend(d[s], y0, x0, fy, fx)
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
