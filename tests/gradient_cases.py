"""Inputs and fp64 references of tests/test_gradients.py (GPU) and tests/test_gradients_cpu.py (TEST HELPER, not
collected): the compositing, plane-fit / depth->points and hash-grid cases, each built once from a fixed seed, and the
same operations evaluated by oracle/ in a chosen dtype with torch autograd.  The CPU module checks these references and
inputs on their own (fp32 evaluation within the tolerance, conditioning, exact lattice); the GPU module holds the HIP
kernels to them."""
import functools

import numpy as np
import torch

from oracle import nerf_oracle as O
from oracle import hashgrid_oracle as HO
from oracle.weights import bench_like_rays

U = 2.0 ** -24                                            # unit roundoff of fp32

# ---------------------------------------------------------------------------------------------- compositing
# every DISPATCH_ITEMS instantiation of csrc/composite.hip (S <= 64 / 128 / 256 / 512 -> 1 / 2 / 4 / 8 samples per lane),
# both sides of each boundary, last lanes with 1 .. ITEMS-1 valid samples
COMPOSITE_S = (2, 7, 63, 64, 65, 128, 129, 130, 256, 257, 300, 511, 512)
COMPOSITE_OUTPUTS = ('rgb', 'disp', 'acc', 'weights', 'depth', 'alpha')      # the order raw2outputs returns them in
COMPOSITE_FLAGS = ((True, False, True), (False, True, False), (False, False, True), (True, True, False))   # white, detach, noise given
COMPOSITE_SUBSETS = (COMPOSITE_OUTPUTS, ('rgb',), ('disp',), ('weights',), ('alpha',), ('acc', 'depth'))
COMPOSITE_RTOL, COMPOSITE_ATOL = 2e-4, 2e-6               # d_raw: test_composite_golden's (atol x nanmax|d_raw_ref|)
COMPOSITE_FWD_RTOL, COMPOSITE_FWD_ATOL = 3e-5, 3e-6       # outputs: test_composite_vs_oracle_sizes'


def composite_items(S):
    return 1 if S <= 64 else 2 if S <= 128 else 4 if S <= 256 else 8


def composite_cases(S):
    """(white, detach, noise given, outputs in the loss) for one S: every flag combination with the full loss, every
    smaller cotangent subset once (flags rotating with S) -- so each runs for every S, hence for every ITEMS."""
    cases = [f + (COMPOSITE_SUBSETS[0],) for f in COMPOSITE_FLAGS]
    for i, sub in enumerate(COMPOSITE_SUBSETS[1:]):
        cases.append(COMPOSITE_FLAGS[(i + S) % 4] + (sub,))
    return cases


@functools.lru_cache(maxsize=None)
def composite_inputs(S, B=19):
    """raw ~ 1.5 N(0,1), sorted z in [1.2, 7.7], bench-like ray directions, noise ~ N(0,1) (the arrays of
    test_composite_vs_oracle_sizes for the same S), cotangents ~ N(0,1) for all six outputs; for B >= 5 the first
    five rays are the fixed rows (noise 0 there, so they hold with and without noise):
      0  every sigma negative                      (acc = 0, disp = NaN)
      1  one saturated sample mid-ray              (sigma = 3e4 over a step >= 0.05: e = 0, t = 1e-10 in fp32 and fp64)
      2  two adjacent saturated samples            (S >= 4)
      3  three coinciding depths                   (S >= 4)
      4  a last sample with negative sigma"""
    rs = np.random.RandomState(S)
    raw = (rs.normal(size=(B, S, 4)) * 1.5).astype(np.float32)
    z = np.sort(rs.uniform(1.2, 7.7, size=(B, S)), -1).astype(np.float32)
    rows = bench_like_rays(B, seed=S)
    noise = rs.normal(size=(B, S)).astype(np.float32)
    if B >= 5:
        noise[:5] = 0
        raw[0, :, 3] = -(np.abs(raw[0, :, 3]) + 0.1)
        m = S // 2 if S > 2 else 0
        raw[1, m, 3] = 3e4
        z[1, m + 1:] += np.float32(0.05)
        if S >= 4:
            m = S // 2 - 1
            raw[2, m:m + 2, 3] = 3e4
            z[2, m + 1:] += np.float32(0.05)
            z[2, m + 2:] += np.float32(0.05)
            j = S // 3
            z[3, j:j + 3] = z[3, j]
        raw[4, -1, 3] = -0.7
    assert (np.diff(z, axis=-1) >= 0).all()
    cs = np.random.RandomState(7000 + S)
    cot = {'rgb': cs.normal(size=(B, 3)), 'disp': cs.normal(size=B), 'acc': cs.normal(size=B), 'depth': cs.normal(size=B),
           'weights': cs.normal(size=(B, S)), 'alpha': cs.normal(size=(B, S))}
    out = {'raw': raw, 'z': z, 'rows': rows, 'noise': noise}
    out.update({'g_' + k: v.astype(np.float32) for k, v in cot.items()})
    for v in out.values():
        v.setflags(write=False)
    return out


def composite_loss(outs, cots, subset):
    """sum over the outputs in `subset` of <output, cotangent>; disp masked to its finite entries (as
    test_composite_golden does: an acc = 0 ray has disp = NaN).  outs / cots: dicts of tensors by output name."""
    loss = 0.
    for name in subset:
        o = outs[name]
        if name == 'disp':
            o = torch.where(torch.isfinite(o), o, torch.zeros_like(o))
        loss = loss + (o * cots[name]).sum()
    return loss


@functools.lru_cache(maxsize=None)
def composite_reference(S, B, white, detach, use_noise, subset, dtype=torch.float64):
    """oracle.nerf_oracle.raw2outputs on the fp32 inputs converted to `dtype`, d_raw by autograd.
    -> ({name: output}, d_raw), numpy arrays in `dtype`."""
    inp = composite_inputs(S, B)
    t = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in inp.items()}
    raw = t['raw'].requires_grad_(True)
    outs = dict(zip(COMPOSITE_OUTPUTS, O.raw2outputs(raw, t['z'], t['rows'][:, 3:6], t['noise'] if use_noise else None,
                                                     white, detach)))
    composite_loss(outs, {k: t['g_' + k] for k in COMPOSITE_OUTPUTS}, subset).backward()
    return {k: v.detach().numpy() for k, v in outs.items()}, raw.grad.numpy()


# ---------------------------------------------------------------------------------------------- plane-fit normals
# windows clipped on all four sides at once (k > H or k > W), H or W = 1, widths of several 256-thread blocks
NORMAL_SHAPES = ((5, 7, 3), (9, 64, 5), (40, 33, 31), (3, 3, 5), (17, 1, 7), (33, 65, 9), (2, 300, 3))
NORMAL_COND_CAP = 1e3                                     # 2-norm condition of every pixel's 3x3 moment matrix
NORMAL_FWD_RTOL, NORMAL_FWD_ATOL = 5e-4, 5e-5             # test_normal_fit_shapes' (atol x max|ref|)
NORMAL_BWD_RTOL, NORMAL_BWD_ATOL = 2e-3, 2e-4             # test_normal_fit_golden's (atol x max|grad_ref|)
DEPTH_SHAPES = ((54, 72), (1, 300), (7, 1), (33, 65))
CHAIN_SHAPE = (9, 64, 5)


@functools.lru_cache(maxsize=None)
def normal_inputs(H, W):
    """points [3,H,W] ~ N(0,1), z + 4 (test_normal_fit_shapes' arrays for the same shape) and a cotangent ~ N(0,1)."""
    rs = np.random.RandomState(H * W)
    pts = rs.normal(size=(3, H, W)).astype(np.float32)
    pts[2] += 4.0
    g = np.random.RandomState(9000 + H * W).normal(size=(3, H, W)).astype(np.float32)
    pts.setflags(write=False)
    g.setflags(write=False)
    return pts, g


def moment_condition(points, k):
    """2-norm condition number of the 3x3 window moment matrix sum p p^T of every pixel; points [3,H,W] -> [H,W]."""
    P = torch.tensor(np.array(points)).double()[None]
    x, y, z = P[:, 0:1], P[:, 1:2], P[:, 2:3]
    mom = torch.cat([x * x, x * y, x * z, y * y, y * z, z * z], 1)
    box = torch.nn.functional.avg_pool2d(mom, k, stride=1, padding=(k - 1) // 2, count_include_pad=True)[0].numpy()
    M = np.stack([box[[0, 1, 2]], box[[1, 3, 4]], box[[2, 4, 5]]], 0)            # [3,3,H,W]
    return np.linalg.cond(M.transpose(2, 3, 0, 1))


@functools.lru_cache(maxsize=None)
def normal_reference(H, W, k, round_sums=False):
    """oracle.nerf_oracle.normal_fit_boxsum kept in fp64 to the end -> (normals, d_points), float64 [3,H,W].
    round_sums: with the nine box sums rounded to fp32 on the way (the CPU module's measure of that storage alone)."""
    pts, g = normal_inputs(H, W)
    P = torch.from_numpy(pts.copy()).double().requires_grad_(True)
    n = O.normal_fit_boxsum(P[None], k, keep_double=True, round_sums=round_sums)[0]
    (n * torch.from_numpy(g.copy()).double()).sum().backward()
    return n.detach().numpy(), P.grad.numpy()


def intrinsics(H, W, f=(41.25, 38.5)):
    """fx != fy, an off-centre non-integer principal point; float32 values (what the C ABI receives), as a 3x3 K."""
    K = np.eye(3, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = f[0], f[1], 0.5 * W + 0.37, 0.5 * H - 1.21
    return K


@functools.lru_cache(maxsize=None)
def depth_inputs(H, W):
    """depth ~ U(1, 6) [H,W], K (float32), cotangent ~ N(0,1) [H,W,3]."""
    rs = np.random.RandomState(5000 + H * W)
    depth = rs.uniform(1.0, 6.0, size=(H, W)).astype(np.float32)
    g = rs.normal(size=(H, W, 3)).astype(np.float32)
    K = intrinsics(H, W)
    for a in (depth, g, K):
        a.setflags(write=False)
    return depth, K, g


def depth_reference(H, W, dtype=torch.float64):
    """oracle.nerf_oracle.depth2xyz in `dtype` -> (points [H,W,3], d_depth [H,W])."""
    depth, K, g = depth_inputs(H, W)
    d = torch.from_numpy(depth.copy()).to(dtype).requires_grad_(True)
    pts = O.depth2xyz(d, torch.from_numpy(K.copy()).to(dtype))
    (pts * torch.from_numpy(g.copy()).to(dtype)).sum().backward()
    return pts.detach().numpy(), d.grad.numpy()


def depth_grad_bound(H, W):
    """Per pixel 4 u (|g_x (w - cx) / fx| + |g_y (h - cy) / fy| + |g_z|): each product term of
    g_x (w - cx) / fx + g_y (h - cy) / fy + g_z carries three fp32 roundings and one or two of the additions."""
    _, K, g = depth_inputs(H, W)
    K = K.astype(np.float64)
    g = g.astype(np.float64)
    ww, hh = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    return 4 * U * (np.abs(g[..., 0] * (ww - K[0, 2]) / K[0, 0]) + np.abs(g[..., 1] * (hh - K[1, 2]) / K[1, 1])
                    + np.abs(g[..., 2]))


# The chain depth -> points -> normals.  Points made by depth2xyz lie on the pixel rays z (a, b, 1), a = (w - cx) / fx, so a
# window's moment matrix sum z^2 r r^T is conditioned by the ray directions alone, ~ (1 + a^2 + b^2)^2 / var_window(a):
# at W = 64, k = 5 that is >= 2e3 for any focal length (x8 in the clipped corner windows), and the 1e3 cap of the point-cloud
# cases cannot hold.  These intrinsics sit near that floor; the CPU module asserts the cap below and that rounding the nine
# box sums to fp32 -- the kernel's storage format -- moves normals and gradient by less than half the tolerances.
CHAIN_F = (24.0, 4.0)
CHAIN_COND_CAP = 2e4


@functools.lru_cache(maxsize=None)
def chain_inputs():
    H, W, k = CHAIN_SHAPE
    rs = np.random.RandomState(31)
    depth = rs.uniform(1.0, 6.0, size=(H, W)).astype(np.float32)
    g = rs.normal(size=(3, H, W)).astype(np.float32)
    K = np.eye(3, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = CHAIN_F[0], CHAIN_F[1], 0.5 * W - 0.37, 0.5 * H + 0.21
    for a in (depth, g, K):
        a.setflags(write=False)
    return depth, K, g


@functools.lru_cache(maxsize=None)
def chain_reference(round_sums=False):
    """-> (points [3,H,W], normals [3,H,W], d_depth [H,W]) of the whole chain in fp64."""
    depth, K, g = chain_inputs()
    d = torch.from_numpy(depth.copy()).double().requires_grad_(True)
    P = O.depth2xyz(d, torch.from_numpy(K.copy()).double()).permute(2, 0, 1)
    n = O.normal_fit_boxsum(P[None], CHAIN_SHAPE[2], keep_double=True, round_sums=round_sums)[0]
    (n * torch.from_numpy(g.copy()).double()).sum().backward()
    return P.detach().numpy(), n.detach().numpy(), d.grad.numpy()


# ---------------------------------------------------------------------------------------------- hash grid
# A 16-level table with INTEGER scales: for x = j / 128 the position x * scale + 0.5 = (j scale + 64) / 128 and the eight
# corner weights (products of three multiples of 1/128) are exact in fp32, contracted into an FMA or not -- so the
# kernel's cells and weights ARE the reference's, on the hashed levels too.  Small tables force many contributions per
# entry; the >= 2^16 ones see more distinct entries per tile than the backward's LDS map has slots.
LATTICE_SCALES = (1, 2, 3, 7, 15, 16, 31, 40, 63, 100, 255, 1000, 4095, 8191, 32767, 65535)
LATTICE_CAPS = (8, 32, 64, 512, 4096, 4096, 1 << 12, 68928, 1 << 12, 1 << 16, 1 << 12, 1 << 16, 1 << 12, 1 << 17, 1 << 12, 1 << 16)
LATTICE_ENTRIES = 425896
LATTICE_DENSE = (0, 1, 2, 3, 4, 7)
LATTICE_P = 4096 + 256 + 37            # two backward tiles (HG_TILE = 4096), a ragged last tile, a ragged last 256-block
LATTICE_P_SMALL = 300                  # a single partial tile


def lattice_levels():
    """[16,4] int32 words {scale (fp32 bits), resolution, offset, size} and the entry count."""
    rows, offset = [], 0
    for scale, cap in zip(LATTICE_SCALES, LATTICE_CAPS):
        res = scale + 1
        size = min((res ** 3 + 7) // 8 * 8, cap)
        rows.append((int(np.float32(scale).view(np.int32)), res, offset, size))
        offset += size
    return np.array(rows, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(16, 4), offset


@functools.lru_cache(maxsize=None)
def lattice_inputs(P):
    """j [P,3] integers in 0..128 (x = j/128: the faces 0 and 1 and exact vertices occur), table ~ N(0,1) float32
    [n,2], dout ~ N(0,1) float32 [32,P] with both feature rows of ~10 % of the (level, point) pairs zero."""
    levels, n = lattice_levels()
    rs = np.random.RandomState(4000 + P)
    j = rs.randint(0, 129, size=(P, 3))
    j[0], j[1], j[2], j[3] = (0, 0, 0), (128, 128, 128), (64, 64, 64), (64, 0, 128)      # (64,64,64): a vertex at odd scales
    table = rs.normal(size=(n, 2)).astype(np.float32)
    dout = rs.normal(size=(32, P)).astype(np.float32)
    skip = rs.uniform(size=(16, P)) < 0.1
    dout[np.repeat(skip, 2, axis=0)] = 0
    for a in (levels, j, table, dout, skip):
        a.setflags(write=False)
    return levels, j, table, dout, skip


@functools.lru_cache(maxsize=None)
def lattice_reference(P, dtype=torch.float64):
    """oracle.hashgrid_oracle.grid_encode in `dtype` on the lattice case.  Returns a dict of numpy arrays:
      f [32,P]       the features                      fabs [32,P]   sum_k |w_k t_k| behind each feature
      grad [n,2]     the table gradient of <f, dout>   A [n,2]       sum |w g| over the contributions to each entry
      count [n]      contributions to each entry from (level, point) pairs whose dout is not skipped"""
    levels, j, table, dout, skip = lattice_inputs(P)
    x = (torch.from_numpy(j.copy()).to(torch.float64) / 128.0).to(dtype)
    t = torch.from_numpy(table.copy()).to(dtype).requires_grad_(True)
    d = torch.from_numpy(dout.copy()).to(dtype).T
    f = HO.grid_encode(x, t, levels)
    (f * d).sum().backward()
    ta = torch.from_numpy(np.abs(table)).to(dtype).requires_grad_(True)
    fabs = HO.grid_encode(x, ta, levels)
    (fabs * d.abs()).sum().backward()
    tc = torch.zeros(table.shape, dtype=torch.float64, requires_grad=True)
    live = torch.from_numpy(np.repeat(~skip, 2, axis=0).T.astype(np.float64))
    (HO.grid_encode(x.double(), tc, levels, unit_weights=True) * live).sum().backward()
    return {'f': f.detach().numpy().T, 'fabs': fabs.detach().numpy().T, 'grad': t.grad.numpy(), 'A': ta.grad.numpy(),
            'count': np.rint(tc.grad.numpy()[:, 0]).astype(np.int64)}


def lattice_forward_bound(ref):
    """|got - ref| <= 8 u sum_k |w_k t_k| + u |ref|: exact weights, eight rounded products and seven rounded additions
    on partial sums below sum |w t|, against the fp64 value rounded once."""
    return 8 * U * ref['fabs'] + U * np.abs(ref['f'])


def lattice_backward_bound(ref):
    """|got - ref| <= (n_e + 2) u A_e: n_e rounded products w g, n_e - 1 rounded additions in any order (LDS or global
    atomics) on partial sums below A_e, and the flush of up to two tiles' sums into the entry."""
    return (ref['count'][:, None] + 2) * U * ref['A']
