"""The definition of reference-view propagation (backward depth warping), restated in numpy: what csrc/warp.hip computes,
in the precision `dtype` (np.float64: the yardstick; np.float32: the kernel's own arithmetic, operation for operation).

Conventions (get_rays', csrc/rays.hip): no half-pixel offset, c2w [3, 4] row-major = [R | o]; the ray parameter is the planar
depth t, a camera-space point is t * ((x - W/2) / f, -(y - H/2) / f, -1); disparity = 1 / t.

Per target n and pixel (y, x) with tgt_mask set and a finite tgt_disp > 0:
    t   = 1 / disp
    dx  = (x - W * .5) / f,  dy = -((y - H * .5) / f),  p_c = (t * dx, t * dy, -t)
    p_w[c] = ((p_c[0] R[c][0] + p_c[1] R[c][1]) + p_c[2] R[c][2]) + o[c]
  for k = 0 .. S-1, s = order[n][k] (skipped unless 0 <= s < S), until a source is taken:
    dl  = p_w - o_s,   q[j] = (R_s[0][j] dl[0] + R_s[1][j] dl[1]) + R_s[2][j] dl[2],   t_s = -q[2]
    u   = (f q[0]) / t_s + W * .5,   v = -((f q[1]) / t_s) + H * .5
    in range:  t_s > 0,  0 <= u <= W - 1,  0 <= v <= H - 1        (a NaN fails every comparison)
    x0  = min(floor(u), W - 2),  y0 = min(floor(v), H - 2),  fx = u - x0,  fy = v - y0,  gx = 1 - fx,  gy = 1 - fy
    a   = (a[y0][x0] gx + a[y0][x0+1] fx) gy + (a[y0+1][x0] gx + a[y0+1][x0+1] fx) fy      each row first, then the two rows;
          the same weights for the source's disparity d_s and its three colour channels
    resid = t_s d_s - 1
    taken iff in range, d_s finite and > 0, |resid| <= tol, the three colours finite
Outputs rgb [N, H, W, 3], index [N, H, W] int32 (the source, or -1), resid [N, H, W]; 0 / -1 / 0 wherever no source is taken.
"""
import numpy as np

M_T = 2.0 ** -16           # margins of the exclusion rule (warp(..., details=True))
M_R = 2.0 ** -16


def default_order(N, S):
    return np.tile(np.arange(S, dtype=np.int32), (N, 1)).reshape(N, S)


def _bilinear(a, y0, x0, fy, fx, one):
    gx, gy = one - fx, one - fy
    if a.ndim == 3:
        fx, fy, gx, gy = fx[:, None], fy[:, None], gx[:, None], gy[:, None]
    top = a[y0, x0] * gx + a[y0, x0 + 1] * fx
    bot = a[y0 + 1, x0] * gx + a[y0 + 1, x0 + 1] * fx
    return top * gy + bot * fy


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
    one, half, m_uv = T(1), T(.5), 2.0 ** -18 * max(H, W)
    rgb, index, resid = np.zeros((N, H, W, 3), T), np.full((N, H, W), -1, np.int32), np.zeros((N, H, W), T)
    excluded = np.zeros((N, H, W), bool)
    for n in range(N):
        d = tgt_disp[n]
        with np.errstate(invalid='ignore'):
            ys, xs = np.nonzero(tgt_mask[n] & np.isfinite(d) & (d > 0))
        t = one / d[ys, xs]
        dx = (xs.astype(T) - T(W) * half) / f
        dy = -((ys.astype(T) - T(H) * half) / f)
        pc = (t * dx, t * dy, -t)
        R, o = tgt_pose[n, :, :3], tgt_pose[n, :, 3]
        pw = [((pc[0] * R[c, 0] + pc[1] * R[c, 1]) + pc[2] * R[c, 2]) + o[c] for c in range(3)]
        got_i, got_c, got_e = np.full(len(ys), -1, np.int32), np.zeros((len(ys), 3), T), np.zeros(len(ys), T)
        marginal = np.zeros(len(ys), bool)
        for k in range(S):
            s = int(order[n, k])
            sel = np.nonzero(got_i < 0)[0]
            if not 0 <= s < S or sel.size == 0:
                continue
            Rs, os_ = src_pose[s, :, :3], src_pose[s, :, 3]
            dl = [pw[c][sel] - os_[c] for c in range(3)]
            q = [(Rs[0, j] * dl[0] + Rs[1, j] * dl[1]) + Rs[2, j] * dl[2] for j in range(3)]
            ts = -q[2]
            with np.errstate(all='ignore'):
                u = (f * q[0]) / ts + T(W) * half
                v = -((f * q[1]) / ts) + T(H) * half
                inr = (ts > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                # out of range: never taken; the taps are clamped into the image so that the details below can look at them
                uc, vc = np.where(np.isfinite(u), u, 0), np.where(np.isfinite(v), v, 0)
                x0 = np.clip(np.floor(uc), 0, W - 2).astype(np.int64)
                y0 = np.clip(np.floor(vc), 0, H - 2).astype(np.int64)
                fx, fy = u - x0.astype(T), v - y0.astype(T)
                ds = _bilinear(src_disp[s], y0, x0, fy, fx, one)
                col = _bilinear(src_rgb[s], y0, x0, fy, fx, one)
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


def pose(angles=(0., 0., 0.), origin=(0., 0., 0.)):
    """c2w [3, 4] fp32: rotations about x, y, z (radians) composed as Rz Ry Rx, and the camera centre."""
    ax, ay, az = angles
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(origin, np.float64)[:, None]], 1).astype(np.float32)


def pixel_rays(c2w, H, W, focal):
    """fp64 origins o [3] and directions d [H, W, 3] of the pixel rays in world space (planar depth: point = o + t d)."""
    c2w = np.asarray(c2w, np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dirs = np.stack([(x - W * .5) / focal, -(y - H * .5) / focal, -np.ones_like(x)], -1)
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
