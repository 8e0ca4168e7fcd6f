"""The definition of the quantile termination depth of a ray, restated in numpy and Python integers: what
csrc/ray_depth.hip computes, word for word.

Per ray with S samples in ASCENDING depth z_0 <= ... <= z_{S-1}, weights w_j, and per level q:
    Lq  = (int64) floor((double) q * 2^40)                    a level must have 0 < q < 1 and Lq >= 1 (q enters as fp32)
    W_j = (int64) floor(clamp((double) w_j, 0, 1) * 2^40)     C_j = sum_{i <= j} W_i in 64-bit integers, C_{-1} = 0
    k   = the smallest j with C_j >= Lq
    no k:       depth = +inf       (the ray never accumulates q)
    k = S - 1:  depth = z_{S-1}    (the last sample owns an unbounded interval, as in compositing)
    otherwise:  f = (double)(Lq - C_{k-1}) / (double) W_k
                depth = (float)((double) z_k + f * ((double) z_{k+1} - (double) z_k))
A ray with any non-finite weight gets NaN at every level.  A non-finite z at the crossing propagates by the arithmetic.
Integer addition is associative, so the result does not depend on any summation order: a kernel agrees bit for bit.
"""
import numpy as np

FIX = 2.0 ** 40
MAX_SAMPLES = 4096
MAX_LEVELS = 8


def level_units(levels):
    """[Lq] as Python ints; ValueError for a level outside 0 < q < 1 or with Lq < 1, or for a count outside 1..8."""
    lv = [np.float32(q) for q in levels]
    if not 1 <= len(lv) <= MAX_LEVELS:
        raise ValueError(f'1..{MAX_LEVELS} levels expected, got {len(lv)}')
    out = []
    for q in lv:
        L = int(np.floor(np.float64(q) * FIX)) if np.isfinite(q) else 0
        if not (0 < q < 1) or L < 1:
            raise ValueError(f'level {q}: 0 < q < 1 and floor(q 2^40) >= 1 expected')
        out.append(L)
    return out


def quantile_depth(z, weights, levels=(0.5,)):
    """depth [B, Q] fp32 of z [B, S], weights [B, S] (fp32 values)."""
    z, w = np.asarray(z, np.float32), np.asarray(weights, np.float32)
    assert z.ndim == 2 and z.shape == w.shape and 1 <= z.shape[1] <= MAX_SAMPLES
    L = level_units(levels)
    B, S = z.shape
    out = np.empty((B, len(L)), np.float32)
    with np.errstate(invalid='ignore'):
        W = np.floor(np.clip(np.where(np.isfinite(w), w, 0).astype(np.float64), 0.0, 1.0) * FIX).astype(np.int64)
    C = np.cumsum(W, axis=1, dtype=np.int64)
    z64 = z.astype(np.float64)
    for b in range(B):
        if not np.isfinite(w[b]).all():
            out[b] = np.nan
            continue
        for i, Lq in enumerate(L):
            k = int(np.searchsorted(C[b], Lq, side='left'))          # the smallest j with C_j >= Lq (C is non-decreasing)
            if k >= S:
                out[b, i] = np.inf
            elif k == S - 1:
                out[b, i] = z[b, k]
            else:
                prev = int(C[b, k - 1]) if k > 0 else 0
                f = np.float64(Lq - prev) / np.float64(W[b, k])
                with np.errstate(invalid='ignore', over='ignore'):
                    out[b, i] = np.float32(z64[b, k] + f * (z64[b, k + 1] - z64[b, k]))
    return out


def expected_depth(z, weights):
    """sum(w z) / sum(w) in fp64: what compositing calls the depth (for the comparison with the median)."""
    z, w = np.asarray(z, np.float64), np.asarray(weights, np.float64)
    return (w * z).sum(-1) / w.sum(-1)


def composite_weights(sigma, z):
    """fp32 weights [B, S] of densities sigma [B, S] along depths z [B, S]: alpha_j = 1 - exp(-sigma_j (z_{j+1} - z_j)), the
    last interval 1e10, w_j = alpha_j prod_{i<j} (1 - alpha_i).  fp64 inside; only a source of realistic rows for the tests."""
    sigma, z = np.asarray(sigma, np.float64), np.asarray(z, np.float64)
    d = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), 1e10)], 1)
    alpha = 1.0 - np.exp(-np.maximum(sigma, 0.0) * d)
    T = np.cumprod(np.concatenate([np.ones((z.shape[0], 1)), 1.0 - alpha[:, :-1] + 1e-10], 1), 1)
    return (alpha * T).astype(np.float32)


def random_rays(B, S, seed):
    """(z [B, S] ascending, weights [B, S]) fp32: densities drawn so that the accumulated weight spreads over (0, 1) -- some rays
    saturate early, some never reach 0.16 -- with stretches of exactly zero weight."""
    rs = np.random.RandomState(seed)
    z = np.sort(rs.uniform(2.0, 6.0, (B, S)).astype(np.float32), axis=1)
    scale = 10.0 ** rs.uniform(-2.5, 1.5, (B, 1))
    sigma = rs.exponential(1.0, (B, S)) * scale * (rs.uniform(size=(B, S)) < 0.5)
    if S > 1:
        sigma[:, -1] *= rs.uniform(size=B) < 0.5          # half of the rays end in empty space: acc < 1
    w = composite_weights(sigma, z)
    if S == 1:
        w[:] = rs.uniform(0.0, 1.0, (B, 1)).astype(np.float32)
    return z, w


def hand_rays():
    """The hand-computed rays of tests/test_ray_depth_cpu.py as one batch of six rays on linspace(2, 6, 8): (z, weights)."""
    z = np.tile(np.linspace(2, 6, 8).astype(np.float32), (6, 1))
    w = np.zeros((6, 8), np.float32)
    w[0, 0], w[0, 7] = 0.55, 0.45                        # two surfaces
    w[1, :3] = 0.25, 0.25, 0.5                           # an exact tie C_1 = Lq at q = 0.5
    w[2, 7] = 1.0                                        # the crossing is the last sample
    w[3, 2] = 0.1                                        # never reaches the levels
    w[4, 4], w[4, 5] = 0.5, 0.5                          # leading zeros
    w[5, 3], w[5, 1] = np.nan, 0.9                       # a NaN weight
    return z, w
