"""The definition of reference-view propagation (backward depth warping), restated in numpy: what csrc/warp.hip computes,
in the precision `dtype` (np.float64: the yardstick; np.float32: the kernel's own arithmetic, operation for operation).

The camera (unproject, project, in_image, lower_footprint, lower_blend and their conventions) is tests/camera_numpy.py's.

Per target n and pixel (y, x) with tgt_mask set and a finite tgt_disp > 0:
    p_w = unproject(pose_n, x, y, t = 1 / disp)
  for k = 0 .. S-1, s = order[n][k] (skipped unless 0 <= s < S), until a source is taken:
    (u, v, t_s) = project(pose_s, p_w);  in range: in_image(t_s, u, v)
    a   = lower_blend on the lower_footprint of (u, v): the same weights for the source's disparity d_s and its three colour
          channels
    resid = t_s d_s - 1
    taken iff in range, d_s finite and > 0, |resid| <= tol, the three colours finite
Outputs rgb [N, H, W, 3], index [N, H, W] int32 (the source, or -1), resid [N, H, W]; 0 / -1 / 0 wherever no source is taken.
"""
import numpy as np

import camera_numpy as C
from camera_numpy import pose                        # noqa: F401  (the cases' poses; imported from here by the tests)

M_T = 2.0 ** -16           # margins of the exclusion rule (warp(..., details=True))
M_R = 2.0 ** -16


def default_order(N, S):
    return np.tile(np.arange(S, dtype=np.int32), (N, 1)).reshape(N, S)


def warp(tgt_disp, tgt_pose, tgt_mask, src_rgb, src_disp, src_pose, focal, order=None, tol=0.05, dtype=np.float64, details=False):
    """(rgb, index, resid) in `dtype`; with details=True also `excluded` [N, H, W] bool: the masked pixels one of whose
    examined sources has a decision within a margin (|t_s| < 2^-16; u or v within 2^-18 max(H, W) of 0 / W-1 / H-1;
    ||resid| - tol| < 2^-16), for which a run in another precision may choose differently.  focal and tol enter as the fp32
    values the kernel receives."""
    T = dtype
    tgt_disp, tgt_pose = np.asarray(tgt_disp, np.float32).astype(T), np.asarray(tgt_pose, np.float32).astype(T)
    src_rgb, src_disp = np.asarray(src_rgb, np.float32).astype(T), np.asarray(src_disp, np.float32).astype(T)
    src_pose = np.asarray(src_pose, np.float32).astype(T)
    tgt_mask = np.asarray(tgt_mask) != 0
    N, H, W = tgt_disp.shape
    S = src_disp.shape[0]
    order = default_order(N, S) if order is None else np.asarray(order)
    assert tgt_pose.shape == (N, 3, 4) and tgt_mask.shape == (N, H, W) and order.shape == (N, S) and H >= 2 and W >= 2
    assert src_rgb.shape == (S, H, W, 3) and src_disp.shape == (S, H, W) and src_pose.shape == (S, 3, 4)
    f, tol = T(np.float32(focal)), T(np.float32(tol))
    one, m_uv = T(1), 2.0 ** -18 * max(H, W)
    rgb, index, resid = np.zeros((N, H, W, 3), T), np.full((N, H, W), -1, np.int32), np.zeros((N, H, W), T)
    excluded = np.zeros((N, H, W), bool)
    for n in range(N):
        d = tgt_disp[n]
        with np.errstate(invalid='ignore'):
            ys, xs = np.nonzero(tgt_mask[n] & np.isfinite(d) & (d > 0))
        pw = C.unproject(T, tgt_pose[n], H, W, f, xs, ys, one / d[ys, xs])
        got_i, got_c, got_e = np.full(len(ys), -1, np.int32), np.zeros((len(ys), 3), T), np.zeros(len(ys), T)
        marginal = np.zeros(len(ys), bool)
        for k in range(S):
            s = int(order[n, k])
            sel = np.nonzero(got_i < 0)[0]
            if not 0 <= s < S or sel.size == 0:
                continue
            u, v, ts = C.project(T, src_pose[s], f, H, W, [pw[c][sel] for c in range(3)])
            with np.errstate(all='ignore'):
                inr = C.in_image(ts, u, v, H, W)
                x0, y0, fx, fy = C.lower_footprint(u, v, H, W)         # out of range: never taken, but the details look at the taps
                ds = C.lower_blend(src_disp[s], y0, x0, fy, fx)
                col = C.lower_blend(src_rgb[s], y0, x0, fy, fx)
                res = ts * ds - one
                ok = inr & np.isfinite(ds) & (ds > 0) & (np.abs(res) <= tol) & np.isfinite(col).all(-1)
                if details:
                    uv_out = ~((u >= -m_uv) & (u <= W - 1 + m_uv) & (v >= -m_uv) & (v <= H - 1 + m_uv))
                    uv_near = (np.abs(u) < m_uv) | (np.abs(u - (W - 1)) < m_uv) | (np.abs(v) < m_uv) | (np.abs(v - (H - 1)) < m_uv)
                    r_near = np.abs(np.abs(res) - tol) < M_R
                    marginal[sel] |= (np.abs(ts) < M_T) | ((ts >= M_T) & ~uv_out & (uv_near | r_near))
            take = sel[ok]
            got_i[take], got_c[take], got_e[take] = s, col[ok], res[ok]
        rgb[n, ys, xs], index[n, ys, xs], resid[n, ys, xs] = got_c, got_i, got_e
        excluded[n, ys, xs] = marginal
    return (rgb, index, resid, excluded) if details else (rgb, index, resid)


def yardstick(*args, **kw):
    """The fp64 run, the fp32 run, and the figures the GPU tests assert with: dict(rgb, index, resid, excluded: the fp64 run's;
    e32_rgb / e32_resid: max |fp32 run - fp64 run| over the kept pixels
    on which both runs chose the same source; index32_differs: kept pixels on which they did not)."""
    rgb, index, resid, excluded = warp(*args, dtype=np.float64, details=True, **kw)
    r32, i32, e32 = warp(*args, dtype=np.float32, **kw)
    same = ~excluded & (i32 == index)
    out = {'rgb': rgb, 'index': index, 'resid': resid, 'excluded': excluded,
           'e32_rgb': float(np.abs(r32.astype(np.float64) - rgb)[same].max()) if same.any() else 0.0,
           'e32_resid': float(np.abs(e32.astype(np.float64) - resid)[same].max()) if same.any() else 0.0,
           'index32_differs': int((~excluded & (i32 != index)).sum())}
    for a in (rgb, index, resid, excluded):
        a.setflags(write=False)
    return out


def pixel_rays(c2w, H, W, focal):
    """fp64 origins o [3] and directions d [H, W, 3] of the pixel rays in world space (planar depth: point = o + t d)."""
    c2w = np.asarray(c2w, np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([*C.pixel_dir(np.float64, x, y, H, W, focal), -np.ones_like(x)], -1)
    return c2w[:, 3], dirs @ c2w[:, :3].T


def box_scene_disparity(c2w, H, W, focal, wall_z=-4.0, box_z=-2.5, box_x=(-.4, .5), box_y=(-.3, .4)):
    """Analytic fp64 disparity (1 / planar depth) of the trial scene seen from c2w: the wall z = wall_z and, in front of it, the
    box face z = box_z over box_x x box_y (a rectangle without sides).  Also returns the world points [H, W, 3]."""
    o, d = pixel_rays(c2w, H, W, focal)
    t_wall = (wall_z - o[2]) / d[..., 2]
    t_box = (box_z - o[2]) / d[..., 2]
    pb = o + t_box[..., None] * d
    hit = (t_box > 0) & (pb[..., 0] >= box_x[0]) & (pb[..., 0] <= box_x[1]) & (pb[..., 1] >= box_y[0]) & (pb[..., 1] <= box_y[1])
    t = np.where(hit, t_box, t_wall)
    return 1.0 / t, o + t[..., None] * d


def smooth_image(H, W, seed, noise=0.002):
    """[H, W, 3] fp32 in (0, 1): a few low sinusoids plus `noise` of white noise."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([.5 + .3 * np.sin(x * a + y * b + c) * np.cos(y * a * .7 - c)
                    for a, b, c in ((.21, .13, .3), (.11, .27, 1.1), (.17, .19, 2.3))], -1)
    return (img + noise * rs.randn(H, W, 3)).astype(np.float32)


# ---- cases shared by tests/test_warp_cpu.py and tests/test_warp.py ------------------------------------------------------------------

TRIAL_BOX = dict(wall_z=-4.0, box_z=-2.5, box_x=(-.4, .5), box_y=(-.3, .4))


def trial_scene():
    """48 x 64, f = 60: the wall and the box face seen by two cameras 0.55 apart, each rotated by a few hundredths; analytic
    disparities rounded to fp32, a smooth source image with 0.002 of noise, every target pixel masked."""
    H, W, f = 48, 64, 60.0
    tgt = pose((0.01, -0.03, 0.01), (-0.25, 0.05, 0.0))
    src = pose((0.0, 0.04, 0.02), (0.30, 0.03, 0.02))
    assert abs(np.linalg.norm(tgt[:, 3].astype(np.float64) - src[:, 3]) - 0.55) < 0.005
    td, tp = box_scene_disparity(tgt, H, W, f, **TRIAL_BOX)
    sd, _ = box_scene_disparity(src, H, W, f, **TRIAL_BOX)
    return dict(H=H, W=W, focal=f, tgt_pose=tgt[None], src_pose=src[None], tgt_disp=td.astype(np.float32)[None],
                src_disp=sd.astype(np.float32)[None], src_rgb=smooth_image(H, W, 7)[None], tgt_mask=np.ones((1, H, W), bool),
                tgt_points=tp)


def hidden_from(points, centre, margin=0.05, box_z=-2.5, box_x=(-.4, .5), box_y=(-.3, .4), **_):
    """[H, W] bool: world points behind the box face whose segment to the camera centre crosses the face shrunk by `margin` on
    every side (0.05: more than one source pixel's footprint on the face, 2.5 / 60, so that every bilinear tap of such a
    pixel lies on the box)."""
    c = np.asarray(centre, np.float64)
    lam = (box_z - points[..., 2]) / (c[2] - points[..., 2])
    hit = points + lam[..., None] * (c - points)
    return (points[..., 2] < box_z - 1e-9) & (lam > 0) & (lam < 1) & (hit[..., 0] >= box_x[0] + margin) & (hit[..., 0] <= box_x[1] - margin) \
        & (hit[..., 1] >= box_y[0] + margin) & (hit[..., 1] <= box_y[1] - margin)


def plane_disparity(c2w, H, W, focal, normal, offset):
    """fp64 disparity of the plane normal . p = offset seen from c2w."""
    o, d = pixel_rays(c2w, H, W, focal)
    nrm = np.asarray(normal, np.float64)
    return (d @ nrm) / (offset - o @ nrm)


def homography_case():
    """33 x 47 (no dimension a multiple of 64 or 4), f = 45: one tilted plane seen by two cameras; the interior of the target
    is masked."""
    H, W, f = 33, 47, 45.0
    tgt, src = pose((0.03, 0.05, -0.02), (0.1, -0.05, 0.0)), pose((-0.04, -0.06, 0.03), (-0.2, 0.1, 0.05))
    nrm, off = (0.15, -0.1, 1.0), -3.0
    m = np.zeros((1, H, W), bool)
    m[0, 1:-1, 1:-1] = True
    return dict(H=H, W=W, focal=f, tgt_pose=tgt[None], src_pose=src[None],
                tgt_disp=plane_disparity(tgt, H, W, f, nrm, off).astype(np.float32)[None],
                src_disp=plane_disparity(src, H, W, f, nrm, off).astype(np.float32)[None], src_rgb=smooth_image(H, W, 8)[None], tgt_mask=m)


ARGS = ('tgt_disp', 'tgt_pose', 'tgt_mask', 'src_rgb', 'src_disp', 'src_pose', 'focal')


def args_of(case):
    return tuple(case[k] for k in ARGS)
