"""The definition of TSDF depth-map fusion restated in numpy (TEST HELPER, not collected): what csrc/tsdf.hip computes, in the
precision `dtype` (np.float64: the yardstick; np.float32: the kernel's own arithmetic, operation for operation), and marching
cubes restricted to observed cells (mvip_mcubes_count_valid), built on tests/mc_numpy.py.

The camera (project, in_image and their conventions) is tests/camera_numpy.py's; the lattice is csrc/mcubes.hip's: point
(i, j, k) sits at x0 + i * hx, ..., hx = (x1 - x0) / (nx - 1); tsdf / count [nx, ny, nz], z fastest.

Per lattice point p, the views in ascending order:
    acc = 0, cnt = 0
    for v = 0 .. V-1:
        (u, w, z) = project(pose_v, p)
        xi = floor(u + .5),  yi = floor(w + .5)                    the nearest pixel
        skip unless in_image(z, xi, yi)                            (a NaN fails every comparison)
        skip if a mask is given and mask[v][yi][xi] == 0
        d = disp[v][yi][xi];  skip unless d finite and > 0
        sdf = 1 / d - z;  skip if sdf < -trunc
        acc += min(1, sdf / trunc);  cnt += 1
    tsdf = cnt > 0 ? acc / cnt : 1;   count = cnt
"""
import numpy as np

import camera_numpy as C
import mc_numpy
from warp_numpy import box_scene_disparity, plane_disparity, pose

M_Z = 2.0 ** -16           # margins of the exclusion rule (fuse(..., details=True))
M_S = 2.0 ** -16


def resolution3(resolution):
    return (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)


def lattice(bound_min, bound_max, resolution, dtype):
    """The three coordinate vectors in `dtype`: x0 + i * ((x1 - x0) / (n - 1)), from the fp32 bounds the kernel receives."""
    T = dtype
    lo, hi = np.asarray(bound_min, np.float32).astype(T), np.asarray(bound_max, np.float32).astype(T)
    res = resolution3(resolution)
    return [(lo[a] + np.arange(res[a]).astype(T) * ((hi[a] - lo[a]) / T(res[a] - 1))).astype(T) for a in range(3)]


def fuse(disp, poses, focal, bound_min, bound_max, resolution, trunc, masks=None, dtype=np.float64, details=False):
    """(tsdf [nx, ny, nz] in `dtype`, count int32); with details=True also `excluded` [nx, ny, nz] bool: the points for which, in
    some view, a decision lies within a margin (|z| < 2^-16; with z >= 2^-16 the fractional part of u + .5 or w + .5 within
    2^-18 max(H, W) of 0 or 1: another pixel, or the image border; on an otherwise seen pixel |sdf + trunc| < 2^-16), so that a
    run in another precision may decide differently.  focal and trunc enter as the fp32 values the kernel receives."""
    T = dtype
    disp = np.asarray(disp, np.float32).astype(T)
    poses = np.asarray(poses, np.float32).astype(T)
    V, H, W = disp.shape
    assert poses.shape == (V, 3, 4)
    if masks is not None:
        masks = np.asarray(masks) != 0
        assert masks.shape == (V, H, W)
    f, tr = T(np.float32(focal)), T(np.float32(trunc))
    one, half, m_uv = T(1), T(.5), 2.0 ** -18 * max(H, W)
    xs, ys, zs = lattice(bound_min, bound_max, resolution, T)
    shape = (len(xs), len(ys), len(zs))
    px, py, pz = (a.reshape(-1) for a in np.meshgrid(xs, ys, zs, indexing='ij'))
    acc, cnt = np.zeros(px.shape[0], T), np.zeros(px.shape[0], np.int32)
    excluded = np.zeros(px.shape[0], bool)
    for v in range(V):
        u, w, z = C.project(T, poses[v], f, H, W, (px, py, pz))
        with np.errstate(all='ignore'):
            su, sw = u + half, w + half
            fx, fy = np.floor(su), np.floor(sw)
            inr = C.in_image(z, fx, fy, H, W)
            xi = np.where(inr, fx, 0).astype(np.int64)
            yi = np.where(inr, fy, 0).astype(np.int64)
            d = disp[v, yi, xi]
            seen = inr & np.isfinite(d) & (d > 0)
            if masks is not None:
                seen &= masks[v, yi, xi]
            sdf = one / d - z
            take = seen & ~(sdf < -tr)
            term = np.minimum(one, sdf / tr)
            if details:
                ru, rw = su - fx, sw - fy
                near_uv = (ru < m_uv) | (ru > 1 - m_uv) | (rw < m_uv) | (rw > 1 - m_uv)
                excluded |= (np.abs(z) < M_Z) | ((z >= M_Z) & near_uv) | (seen & (np.abs(sdf + tr) < M_S))
        acc = np.where(take, acc + np.where(take, term, 0), acc).astype(T)
        cnt = cnt + take.astype(np.int32)
    with np.errstate(all='ignore'):
        tsdf = np.where(cnt > 0, acc / np.maximum(cnt, 1).astype(T), one).astype(T)
    out = (tsdf.reshape(shape), cnt.reshape(shape))
    return out + (excluded.reshape(shape),) if details else out


def yardstick(*args, **kw):
    """The fp64 run, the fp32 run and the figures the tests assert with: dict(tsdf, count, excluded: the fp64 run's; tsdf32,
    count32: the fp32 run's; e32: max |fp32 run - fp64 run| over the points that are not excluded and whose counts agree;
    count32_differs: kept points whose counts do not; excluded_share)."""
    tsdf, count, excluded = fuse(*args, dtype=np.float64, details=True, **kw)
    t32, c32 = fuse(*args, dtype=np.float32, **kw)
    same = ~excluded & (c32 == count)
    out = {'tsdf': tsdf, 'count': count, 'excluded': excluded, 'tsdf32': t32, 'count32': c32,
           'e32': float(np.abs(t32.astype(np.float64) - tsdf)[same].max()) if same.any() else 0.0,
           'count32_differs': int((~excluded & (c32 != count)).sum()), 'excluded_share': float(excluded.mean())}
    for a in (tsdf, count, excluded, t32, c32):
        a.setflags(write=False)
    return out


def mc_lattice(tsdf, count):
    """(g, valid) as mesh.fuse_depths hands them to marching cubes at threshold 1: g = 1 - tsdf, 0 where count == 0."""
    valid = np.asarray(count) > 0
    g = np.where(valid, np.float32(1) - np.asarray(tsdf, np.float32), np.float32(0)).astype(np.float32)
    return g, valid


def live_cells(valid):
    """[nx-1, ny-1, nz-1] bool: the cells whose eight corners are valid."""
    v = np.asarray(valid) != 0
    nx, ny, nz = v.shape
    live = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for corner in range(8):
        dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
        live &= v[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    return live


def edge_live(live):
    """[nx, ny, nz, 3] bool: the owned edge (+x, +y, +z) of each point has at least one live cell among the up to four around it."""
    nx, ny, nz = (n + 1 for n in live.shape)
    pad = np.zeros((nx + 1, ny + 1, nz + 1), bool)                 # pad[i + 1, j + 1, k + 1] = live[i, j, k]; False outside
    pad[1:nx, 1:ny, 1:nz] = live
    c = lambda a, b, cc: pad[1 + a:1 + a + nx, 1 + b:1 + b + ny, 1 + cc:1 + cc + nz]
    out = np.zeros((nx, ny, nz, 3), bool)
    out[..., 0] = c(0, 0, 0) | c(0, -1, 0) | c(0, 0, -1) | c(0, -1, -1)
    out[..., 1] = c(0, 0, 0) | c(-1, 0, 0) | c(0, 0, -1) | c(-1, 0, -1)
    out[..., 2] = c(0, 0, 0) | c(-1, 0, 0) | c(0, -1, 0) | c(-1, -1, 0)
    return out


def marching_cubes_valid(grid, valid, iso, bmin, bmax, return_cells=False):
    """mc_numpy.marching_cubes restricted to observed cells: the triangles of the live cells in (cell, table slot) order and the
    flagged vertices (the values cross and a live cell shares the edge) in (point, axis) order.  -> verts [V, 3] f32, faces
    [F, 3] int64, normals [V, 3] f32 (central differences of `grid` as it is, fill values included); with return_cells also
    the linear cell index of every face."""
    F32, TABLE, COUNTS = mc_numpy.F32, mc_numpy.TABLE, mc_numpy.COUNTS
    v = np.ascontiguousarray(grid, dtype=F32)
    nx, ny, nz = v.shape
    lo, hi = np.asarray(bmin, F32), np.asarray(bmax, F32)
    iso = F32(iso)
    h = ((hi - lo) / np.array([nx - 1, ny - 1, nz - 1], F32)).astype(F32)
    with np.errstate(invalid='ignore'):
        ins = v >= iso
    live = live_cells(valid)
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    cross &= edge_live(live)
    mask = (cross[..., 0] * 1 + cross[..., 1] * 2 + cross[..., 2] * 4).reshape(-1)
    counts = cross.reshape(-1, 3).sum(1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pt, ax = np.nonzero(cross.reshape(-1, 3))
    i, j, k = np.unravel_index(pt, v.shape)
    d = np.eye(3, dtype=np.int64)[ax]
    i1, j1, k1 = i + d[:, 0], j + d[:, 1], k + d[:, 2]
    v0, v1 = v[i, j, k], v[i1, j1, k1]
    t = ((iso - v0) / (v1 - v0)).astype(F32)
    p0 = np.stack([lo[0] + i.astype(F32) * h[0], lo[1] + j.astype(F32) * h[1], lo[2] + k.astype(F32) * h[2]], -1)
    p1 = np.stack([lo[0] + i1.astype(F32) * h[0], lo[1] + j1.astype(F32) * h[1], lo[2] + k1.astype(F32) * h[2]], -1)
    verts = (p0 + t[:, None] * (p1 - p0)).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        G = [mc_numpy._grad(v, a, h[a]) for a in range(3)]
        g0 = np.stack([G[a][i, j, k] for a in range(3)], -1)
        g1 = np.stack([G[a][i1, j1, k1] for a in range(3)], -1)
        g = (g0 + t[:, None] * (g1 - g0)).astype(F32)
        ln = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).astype(F32)
        normals = np.where(ln[:, None] > 0, -g / ln[:, None], F32(0)).astype(F32)
    c = np.where(live, mc_numpy.cube_indices(ins, True), 0)
    ci, cj, ck = np.nonzero(COUNTS[c] > 0)
    cube = c[ci, cj, ck]
    cell = np.ravel_multi_index((ci, cj, ck), v.shape)
    nt = COUNTS[cube]
    rep = np.repeat(np.arange(cube.shape[0]), nt)
    slot = np.arange(rep.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)
    e = TABLE[cube[rep][:, None], 3 * slot[:, None] + np.arange(3)[None]]
    a, r1, r2 = e >> 2, e & 1, (e >> 1) & 1
    dx = np.where(a == 0, 0, r1)
    dy = np.where(a == 1, 0, np.where(a == 0, r1, r2))
    dz = np.where(a == 2, 0, r2)
    m = cell[rep][:, None] + dx * ny * nz + dy * nz + dz
    below = mask[m] & ((1 << a) - 1)
    rank = (below & 1) + ((below >> 1) & 1)
    faces = (first[m] + rank).astype(np.int64).reshape(-1, 3)
    return (verts, faces, normals, cell[rep]) if return_cells else (verts, faces, normals)


def triangles_in_dead_cells(grid, valid, iso):
    """Triangles the unrestricted marching cubes puts into cells that are not live."""
    c = mc_numpy.cube_indices(grid, iso)
    return int(mc_numpy.COUNTS[c][~live_cells(valid)].sum())


# ---- cases shared by tests/test_tsdf_cpu.py and tests/test_tsdf.py ----------------------------------------------------------------
# Generic poses: every angle non-zero and no camera centre on a lattice plane, so that no lattice row sits on a pixel-rounding
# boundary.

TRIAL_BOX = dict(wall_z=-4.0, box_z=-2.5, box_x=(-.4, .5), box_y=(-.3, .4))


def trial_case():
    """48 x 64, f = 60: the wall z = -4 and the box face z = -2.5 of warp_numpy.trial_scene seen by three cameras; lattice
    25 x 19 x 33 = 15,675 points (not a multiple of the 1,024-point workgroup), step 0.1, trunc = four steps."""
    H, W, f = 48, 64, 60.0
    poses = np.stack([pose((0.01, -0.03, 0.01), (-0.253, 0.047, 0.013)), pose((0.013, 0.04, 0.02), (0.307, 0.031, 0.021)),
                      pose((-0.035, 0.012, -0.015), (0.021, -0.262, -0.034))])
    disp = np.stack([box_scene_disparity(p, H, W, f, **TRIAL_BOX)[0] for p in poses]).astype(np.float32)
    return dict(disp=disp, poses=poses, focal=f, bound_min=(-1.2, -0.9, -4.4), bound_max=(1.2, 0.9, -1.2), resolution=(25, 19, 33),
                trunc=0.4)


PLANE_NORMAL, PLANE_OFFSET = (0.15, -0.1, 1.0), -3.0
PLANE_LATTICES = ((17, 13, 21), (33, 25, 41))


def plane_case(resolution=PLANE_LATTICES[0]):
    """33 x 47 (no dimension a multiple of 64), f = 45: the tilted plane of warp_numpy.homography_case seen by three cameras;
    the box [-0.8, 0.8] x [-0.6, 0.6] x [-4, -2] in steps of 0.1 (17 x 13 x 21) or 0.05 (33 x 25 x 41); trunc = four steps."""
    H, W, f = 33, 47, 45.0
    poses = np.stack([pose((0.03, 0.05, -0.02), (0.113, -0.057, 0.011)), pose((-0.04, -0.06, 0.03), (-0.207, 0.103, 0.053)),
                      pose((0.02, -0.015, 0.045), (0.031, 0.171, -0.027))])
    disp = np.stack([plane_disparity(p, H, W, f, PLANE_NORMAL, PLANE_OFFSET) for p in poses]).astype(np.float32)
    lo, hi = (-0.8, -0.6, -4.0), (0.8, 0.6, -2.0)
    step = max((np.float32(hi[a]) - np.float32(lo[a])) / np.float32(resolution[a] - 1) for a in range(3))
    return dict(disp=disp, poses=poses, focal=f, bound_min=lo, bound_max=hi, resolution=tuple(resolution), trunc=4.0 * float(step))


def plane_mesh_figures(verts, normals, case):
    """(the largest distance of a vertex from the plane in units of the smallest lattice step, the smallest cosine between a
    normal and the plane's unit normal on the camera side)."""
    n = np.asarray(PLANE_NORMAL, np.float64)
    ln = np.linalg.norm(n)
    lo, hi, res = np.asarray(case['bound_min'], np.float64), np.asarray(case['bound_max'], np.float64), case['resolution']
    step = min((hi[a] - lo[a]) / (res[a] - 1) for a in range(3))
    dist = np.abs(np.asarray(verts, np.float64) @ n - PLANE_OFFSET) / ln
    # the cameras sit near z = 0, where normal . p - offset = 3 > 0: the camera side is +normal
    cos = np.asarray(normals, np.float64) @ (n / ln)
    return float(dist.max() / step), float(cos.min())


def hit_pixel(case, view):
    """(y, x) of the pixel of `view` that counts for the most lattice points (fp64): a pixel whose disparity matters."""
    H, W = case['disp'].shape[1:]
    one = [case['disp'][view:view + 1], case['poses'][view:view + 1]]
    _, c = fuse(*one, *args_of(case)[2:])
    T = np.float64
    xs, ys, zs = lattice(case['bound_min'], case['bound_max'], case['resolution'], T)
    p = np.stack(np.meshgrid(xs, ys, zs, indexing='ij'), -1).reshape(-1, 3)[c.reshape(-1) > 0]
    _, u, w = C.project_points(p, case['poses'][view], T(np.float32(case['focal'])), H, W)
    xi, yi = np.floor(u + .5).astype(np.int64), np.floor(w + .5).astype(np.int64)
    hits = np.bincount(yi * W + xi, minlength=H * W)
    return int(hits.argmax() // W), int(hits.argmax() % W)


ARGS = ('disp', 'poses', 'focal', 'bound_min', 'bound_max', 'resolution', 'trunc')


def args_of(case):
    return tuple(case[k] for k in ARGS)
