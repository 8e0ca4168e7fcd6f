"""The ray distortion loss (mip-NeRF 360 eq. 15) restated from its definition (csrc/distortion.hip's header), for the tests.

s, m and d are computed in fp32 exactly as the definition says (one correctly rounded operation each, in that order; numpy's
fp32 scalar operations are correctly rounded); everything after that is fp64, as the O(S^2) double sum."""
import numpy as np

F = np.float32


def intervals(z, near, far, lindisp=False):
    """(m, d) in fp32: z [B, S] ascending, near / far [B]."""
    z = np.asarray(z, F)
    near, far = np.asarray(near, F).reshape(-1, 1), np.asarray(far, F).reshape(-1, 1)
    with np.errstate(all='ignore'):
        if lindisp:
            one = F(1.)
            a = one / near
            s = ((one / z).astype(F) - a).astype(F) / ((one / far).astype(F) - a).astype(F)
        else:
            s = (z - near).astype(F) / (far - near).astype(F)
        s = s.astype(F)
        m, d = s.copy(), np.zeros_like(s)
        m[:, :-1] = F(0.5) * (s[:, :-1] + s[:, 1:]).astype(F)
        d[:, :-1] = s[:, 1:] - s[:, :-1]
    assert m.dtype == F and d.dtype == F
    return m, d


def pair_distances(m):
    """|m_i - m_j| in fp64, [B, S, S]."""
    m = np.asarray(m, np.float64)
    with np.errstate(all='ignore'):
        return np.abs(m[:, :, None] - m[:, None, :])


def loss_and_grad(A, d, w):
    """The fp64 double sum on given pair distances A and widths d: L [B], g [B, S]."""
    d, w = np.asarray(d, np.float64), np.asarray(w, np.float64)
    with np.errstate(all='ignore'):
        Aw = np.einsum('bij,bj->bi', A, w)
        L = np.einsum('bi,bi->b', w, Aw) + (w * w * d).sum(1) / 3.0
        g = 2.0 * Aw + (2.0 / 3.0) * w * d
    return L, g


def distortion(z, w, near, far, lindisp=False):
    """(L [B], g [B, S], L_abs, g_abs): the loss, its gradient with respect to w, and the same two formulas with |w| for w."""
    m, d = intervals(z, near, far, lindisp)
    A = pair_distances(m)
    L, g = loss_and_grad(A, d, w)
    L_abs, g_abs = loss_and_grad(A, d, np.abs(np.asarray(w, np.float64)))
    return L, g, L_abs, g_abs
