"""SSIM with its gradient, restated in numpy (the definition of csrc/ssim.hip; a helper of the tests, not a test).

x, y [N, H, W, C], channel-last.  Window: 11 taps g_k = e_k / sum e_k, e_k = exp(-(k-5)^2 / (2 1.5^2)), evaluated and summed in
ascending order in fp64 and rounded to fp32; every run, the fp64 one included, uses these fp32 values.  The filter is separable
and "valid": F(v)(i, j) = sum_a g_a sum_b g_b v(i+a, j+b), taps ascending, along the rows first and then down the columns
(order='rows'; order='cols' is the other way round, for the error floor).  The map is [N, H-10, W-10, C]; map pixel (i, j) is
centred on image pixel (i+5, j+5) and counts iff the mask is set there.

dtype=np.float64 on the fp32 inputs is the yardstick; dtype=np.float32 follows the kernel's operation order.
"""
import math

import numpy as np

TAPS, HALF = 11, 5
C1, C2 = 1e-4, 9e-4


def window(dtype=np.float64):
    e = [math.exp(-((k - 5.0) ** 2) / (2.0 * 1.5 ** 2)) for k in range(TAPS)]
    total = 0.0
    for v in e:
        total += v
    return np.array([v / total for v in e], np.float64).astype(np.float32).astype(dtype)


def _along(v, g, axis):
    n = v.shape[axis] - (TAPS - 1)
    sl = lambda k: tuple(slice(k, k + n) if a == axis else slice(None) for a in range(v.ndim))
    out = g[0] * v[sl(0)]
    for k in range(1, TAPS):
        out = out + g[k] * v[sl(k)]
    return out


def filt(v, dtype, order='rows'):
    """F(v): [N, H, W, C] -> [N, H-10, W-10, C]."""
    g = window(dtype)
    v = np.asarray(v, dtype)
    first, second = (2, 1) if order == 'rows' else (1, 2)
    return _along(_along(v, g, first), g, second)


def terms(x, y, dtype=np.float64, order='rows'):
    """Every intermediate of the formula, per map pixel and channel."""
    x, y = np.asarray(x, np.float32).astype(dtype), np.asarray(y, np.float32).astype(dtype)
    two, c1, c2 = dtype(2.0), dtype(np.float32(C1)) if dtype == np.float32 else dtype(C1), dtype(np.float32(C2)) if dtype == np.float32 else dtype(C2)
    t = dict(mx=filt(x, dtype, order), my=filt(y, dtype, order), exx=filt(x * x, dtype, order), eyy=filt(y * y, dtype, order),
             exy=filt(x * y, dtype, order))
    t['mxx'], t['myy'], t['mxy'] = t['mx'] * t['mx'], t['my'] * t['my'], t['mx'] * t['my']
    t['sxx'], t['syy'], t['sxy'] = t['exx'] - t['mxx'], t['eyy'] - t['myy'], t['exy'] - t['mxy']
    t['n1'], t['n2'] = two * t['mxy'] + c1, two * t['sxy'] + c2
    t['d1'], t['d2'] = (t['mxx'] + t['myy']) + c1, (t['sxx'] + t['syy']) + c2
    t['d12'] = t['d1'] * t['d2']
    t['s'] = (t['n1'] * t['n2']) / t['d12']
    return t


def counted(shape, mask):
    """[N, H-10, W-10] bool: the map pixels that count."""
    N, H, W = shape[:3]
    if mask is None:
        return np.ones((N, H - 2 * HALF, W - 2 * HALF), bool)
    return np.asarray(mask).astype(bool)[:, HALF:H - HALF, HALF:W - HALF]


def ssim(x, y, mask=None, dtype=np.float64, order='rows'):
    """(ssim [N] (dtype), map [N, H-10, W-10, C] (dtype), count [N] int64).  count 0: exactly 1."""
    s = terms(x, y, dtype, order)['s']
    m = counted(np.shape(x), mask)
    count = m.reshape(m.shape[0], -1).sum(1).astype(np.int64)
    C = s.shape[-1]
    total = (s.astype(np.float64) * m[..., None]).reshape(s.shape[0], -1).sum(1)
    mean = np.where(count > 0, total / np.maximum(count * C, 1), 1.0)
    return mean.astype(dtype), s, count


def grad_planes(t, dtype):
    two = dtype(2.0)
    B = -t['s'] / t['d2']
    Cp = (two * t['n1']) / t['d12']
    a1 = ((two * t['my']) * t['n2']) / t['d12'] - ((two * t['mx']) * t['s']) / t['d1']
    a2 = (two * t['mx']) * B
    a3 = t['my'] * Cp
    return (a1 - a2) - a3, B, Cp, (a1, a2, a3)


def _full(p, dtype, order):
    """G(P): the plane zero-padded by 10 on every side, then F: [N, H-10, W-10, C] -> [N, H, W, C]."""
    pad = TAPS - 1
    return filt(np.pad(p, ((0, 0), (pad, pad), (pad, pad), (0, 0))), dtype, order)


def grad(x, y, gout, mask=None, dtype=np.float64, order='rows'):
    """d (sum_n gout_n ssim_n) / d x, [N, H, W, C] (dtype)."""
    t = terms(x, y, dtype, order)
    A, B, Cp, _ = grad_planes(t, dtype)
    m = counted(np.shape(x), mask)
    count = m.reshape(m.shape[0], -1).sum(1)
    C = np.shape(x)[-1]
    w = m[..., None].astype(dtype)
    xs, ys = np.asarray(x, np.float32).astype(dtype), np.asarray(y, np.float32).astype(dtype)
    g = (_full(A * w, dtype, order) + (dtype(2.0) * xs) * _full(B * w, dtype, order)) + ys * _full(Cp * w, dtype, order)
    scale = np.where(count > 0, np.asarray(gout, np.float32).astype(dtype) / np.maximum(count * C, 1).astype(dtype), dtype(0.0)).astype(dtype)
    out = scale[:, None, None, None] * g
    out[count == 0] = 0
    return out.astype(dtype)


def magnitude_map(x, y):
    """M_p = 1 + |s| (E[x^2] + E[y^2] + mu_x^2 + mu_y^2) / d2 + 2 |n1| (|E[xy]| + |mu_x mu_y|) / (d1 d2), fp64: the size of the
    terms that cancel in a map pixel, the unit of its error bound."""
    t = terms(x, y, np.float64)
    return 1.0 + np.abs(t['s']) * (t['exx'] + t['eyy'] + t['mxx'] + t['myy']) / t['d2'] \
        + 2.0 * np.abs(t['n1']) * (np.abs(t['exy']) + np.abs(t['mxy'])) / t['d12']


def magnitude_grad(x, y, gout, mask=None):
    """F_q: the gradient expression with every term replaced by its absolute value (|A| = the sum of the absolute values of its
    own three terms), fp64, [N, H, W, C]."""
    t = terms(x, y, np.float64)
    _, B, Cp, (a1, a2, a3) = grad_planes(t, np.float64)
    m = counted(np.shape(x), mask)
    count = m.reshape(m.shape[0], -1).sum(1)
    C = np.shape(x)[-1]
    w = m[..., None].astype(np.float64)
    xs, ys = np.asarray(x, np.float64), np.asarray(y, np.float64)
    g = _full((np.abs(a1) + np.abs(a2) + np.abs(a3)) * w, np.float64, 'rows') \
        + 2.0 * np.abs(xs) * _full(np.abs(B) * w, np.float64, 'rows') + np.abs(ys) * _full(np.abs(Cp) * w, np.float64, 'rows')
    scale = np.where(count > 0, np.abs(np.asarray(gout, np.float64)) / np.maximum(count * C, 1), 0.0)
    return scale[:, None, None, None] * g


def yardstick(x, y, gout=None, mask=None):
    """The figures of a case: the fp64 run, the fp32 runs' distance to it (per map pixel for the map, the larger of the two
    filter orders for the gradient), the magnitude planes."""
    s64, map64, count = ssim(x, y, mask)
    out = {'ssim': s64, 'map': map64, 'count': count, 'M': magnitude_map(x, y)}
    out['map32_err'] = np.abs(ssim(x, y, mask, np.float32)[1].astype(np.float64) - map64)
    if gout is not None:
        g64 = grad(x, y, gout, mask)
        out['grad'] = g64
        out['e32'] = max(float(np.abs(grad(x, y, gout, mask, np.float32, o).astype(np.float64) - g64).max()) for o in ('rows', 'cols'))
        out['F'] = magnitude_grad(x, y, gout, mask)
    return out
