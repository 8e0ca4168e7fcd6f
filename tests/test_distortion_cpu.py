"""The ray distortion loss without a GPU: the numpy restatement (tests/distortion_numpy.py) against fp64 autograd of its own
loss, the argument checks of the mvip_distortion_loss entry point, and the host side of run.render_rays' `distortion` keyword."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_numpy as D                             # noqa: E402
import occupancy_numpy as R                              # noqa: E402

from mvip_nerf_amd import _lib, run                      # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid        # noqa: E402

OK, EINVAL = 0, -1
P0 = None            # NULL


def raw(name, *args):
    return getattr(_lib.load(), name)(*args)


@pytest.mark.parametrize('lindisp', [False, True])
def test_restated_gradient_equals_fp64_autograd_of_the_restated_loss(lindisp):
    rs = np.random.RandomState(16)
    B, S = 6, 16
    z = np.sort(rs.uniform(1.2, 7.74, (B, S)).astype(np.float32), 1)
    w = rs.rand(B, S).astype(np.float32)
    w[1] = w[1] ** 8
    w[2] = rs.randn(S)                                                          # signs: |m_i - m_j| does not care
    near, far = np.full(B, 1.2, np.float32), np.full(B, 7.74, np.float32)
    L, g, L_abs, g_abs = D.distortion(z, w, near, far, lindisp)
    m, d = D.intervals(z, near, far, lindisp)
    assert (np.diff(m, axis=1) >= 0).all() and (d >= 0).all() and (d[:, -1] == 0).all() and (m[:, -1] <= 1).all()
    wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    mt, dt = torch.from_numpy(m.astype(np.float64)), torch.from_numpy(d.astype(np.float64))
    Lt = (wt[:, :, None] * wt[:, None, :] * (mt[:, :, None] - mt[:, None, :]).abs()).sum((1, 2)) + (wt * wt * dt).sum(1) / 3
    gt, = torch.autograd.grad(Lt.sum(), wt)
    np.testing.assert_allclose(L, Lt.detach().numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(g, gt.numpy(), rtol=1e-9, atol=1e-12)
    assert (L_abs >= np.abs(L)).all() and (g_abs >= np.abs(g) * (1 - 1e-12)).all()
    # S = 1: a point, no spread
    L1, g1, _, _ = D.distortion(z[:, :1], w[:, :1], near, far, lindisp)
    assert (L1 == 0).all() and (g1 == 0).all()


def test_entry_point_argument_checks():
    name = 'mvip_distortion_loss'                  # (rows, ncols, z, weights, B, S, lindisp, loss, grad, stream)
    assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == 10
    assert raw(name, P0, 11, P0, P0, 4, 0, 0, P0, P0, P0) == EINVAL              # S = 0
    assert raw(name, P0, 11, P0, P0, -1, 64, 0, P0, P0, P0) == EINVAL            # B = -1
    assert raw(name, P0, 9, P0, P0, 4, 64, 0, P0, P0, P0) == EINVAL              # ncols = 9
    assert raw(name, P0, 9, P0, P0, 0, 64, 0, P0, P0, P0) == EINVAL              # ... also with no rays
    assert raw(name, P0, 8, P0, P0, 1 << 25, 64, 1, P0, P0, P0) == EINVAL        # B * S = 2^31
    assert raw(name, P0, 8, P0, P0, 1 << 40, 1 << 30, 1, P0, P0, P0) == EINVAL   # B * S past 2^63
    for ncols in (8, 11):
        assert raw(name, P0, ncols, P0, P0, 0, 64, 0, P0, P0, P0) == OK          # no rays, null operands
        assert raw(name, P0, ncols, P0, P0, 4, 64, 1, P0, P0, P0) == EINVAL      # a good shape with null operands


def test_keyword_default_is_off():
    assert inspect.signature(run.render_rays).parameters['distortion'].default is False


def test_distortion_with_occupancy_is_refused():
    from mvip_nerf_amd.run_nerf_helpers import NeRF
    net = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    rows = torch.zeros(4, 11)
    rows[:, 5] = -1.0
    rows[:, 6], rows[:, 7] = 1.0, 2.0
    rows[:, 10] = -1.0

    def qfn(*a):
        raise AssertionError('the network must not be queried')
    occ = np.random.RandomState(0).rand(5, 3, 7) < 0.5
    grid = OccupancyGrid((-1, -2, 0), (1, 2, 0.5), occ.shape, R.pack(occ))
    with torch.no_grad():
        with pytest.raises(ValueError, match='distortion'):
            run.render_rays(rows, net, qfn, N_samples=8, N_importance=8, network_fine=net, occupancy=grid, distortion=True)
    assert grid.stats['network_launches'] == 0
