"""The ray distortion loss on the GPU (csrc/distortion.hip, ops.distortion_loss, run.render_rays' `distortion` keyword,
trainer's `distortion_lambda`): the kernel against the numpy restatement (tests/distortion_numpy.py) within the a-priori
bound of its sums, its bit-level properties (loss-only launch, batch independence, a NaN ray), the autograd plumbing, the
two keys of render_rays against the op on the call's own outputs, and one trainer step.

Measured on an MI355X, the largest fraction of the bound (2S + 8) * 2^-24 * {L_abs, g_abs} over every case below:
loss 0.149, gradient 0.119 (both at S = 2, where the bound is 12 ulp; for S >= 63 at most 0.023 and 0.032)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distortion_numpy as D                             # noqa: E402

import bench                                             # noqa: E402
from mvip_nerf_amd import _lib, ops, run                 # noqa: E402
from mvip_nerf_amd._lib import ptr, stream               # noqa: E402
from mvip_nerf_amd.run_nerf_helpers import _uniforms     # noqa: E402

pytestmark = pytest.mark.gpu

NEAR, FAR = 1.2, 7.74
SHAPES = [(1, 1), (1, 2), (5, 63), (4, 64), (7, 65), (3, 128), (9, 192), (2, 257), (1030, 128)]
KINDS = ('uniform', 'uniform8', 'onehot', 'bump')


def N(t):
    return t.detach().cpu().numpy()


def bits(t):
    return N(t.detach().contiguous().view(torch.int32))


def make_weights(kind, B, S, rs):
    if kind == 'uniform':
        return rs.rand(B, S).astype(np.float32)
    if kind == 'uniform8':
        return (rs.rand(B, S) ** 8).astype(np.float32)
    if kind == 'onehot':
        w = np.zeros((B, S), np.float32)
        w[np.arange(B), rs.randint(0, S, B)] = (0.5 + rs.rand(B)).astype(np.float32)
        return w
    j = np.arange(S)[None]                               # a Gaussian bump at 0.7 S of width 0.02 S on a 1e-4 uniform floor
    return (np.exp(-0.5 * ((j - 0.7 * S) / (0.02 * S)) ** 2) + 1e-4 * rs.rand(B, S)).astype(np.float32)


def make_inputs(B, S, kind, seed, ncols=11):
    """(z, w, rows) as numpy: depths sorted uniform in [near, far]; the row columns the loss does not read hold noise."""
    rs = np.random.RandomState(seed)
    z = np.sort(rs.uniform(NEAR, FAR, (B, S)).astype(np.float32), 1)
    rows = rs.randn(B, ncols).astype(np.float32)
    rows[:, 6], rows[:, 7] = NEAR, FAR
    return z, make_weights(kind, B, S, rs), rows


def kernel(w, z, rows, lindisp, want_grad=True):
    """One launch of the entry point on device tensors: (loss [B], grad [B, S] or None)."""
    B, S = z.shape
    loss = torch.full((B,), -7.0, device=z.device)
    grad = torch.full((B, S), -7.0, device=z.device) if want_grad else None
    _lib.call('mvip_distortion_loss', ptr(rows), rows.shape[1], ptr(z), ptr(w), B, S, int(lindisp), ptr(loss), ptr(grad), stream())
    return loss, grad


_REF = {}


def reference(B, S, kind, lindisp):
    """The restatement of one case, computed once and shared."""
    key = (B, S, kind, lindisp)
    if key not in _REF:
        z, w, rows = make_inputs(B, S, kind, seed=1000 * S + B, ncols=8 if S % 2 else 11)
        _REF[key] = (z, w, rows) + D.distortion(z, w, rows[:, 6], rows[:, 7], lindisp)
    return _REF[key]


@pytest.mark.parametrize('lindisp', [False, True])
@pytest.mark.parametrize('B,S', SHAPES)
def test_kernel_within_the_a_priori_bound_of_the_restatement(B, S, lindisp, cuda):
    for kind in KINDS:
        z, w, rows, L_ref, g_ref, L_abs, g_abs = reference(B, S, kind, lindisp)
        L, g = kernel(*(torch.from_numpy(a).to(cuda) for a in (w, z, rows)), lindisp)
        L, g = N(L).astype(np.float64), N(g).astype(np.float64)
        bound_L, bound_g = (2 * S + 8) * 2.0 ** -24 * L_abs, (2 * S + 8) * 2.0 ** -24 * g_abs
        err_L, err_g = np.abs(L - L_ref), np.abs(g - g_ref)
        frac = lambda e, b: float(np.where(b > 0, e / np.where(b > 0, b, 1), 0).max())
        print(f'distortion-fraction B {B} S {S} lindisp {int(lindisp)} {kind}: loss {frac(err_L, bound_L):.4f} grad {frac(err_g, bound_g):.4f}')
        assert np.isfinite(L).all() and np.isfinite(g).all()
        assert (err_L <= bound_L).all(), (kind, float((err_L - bound_L).max()))      # a zero bound demands an exact zero
        assert (err_g <= bound_g).all(), (kind, float((err_g - bound_g).max()))
        if S == 1:
            assert (L == 0).all() and (g == 0).all()
        elif kind != 'onehot':
            assert (L_ref > 0).any() and (g_ref > 0).any()


@pytest.fixture(scope='module')
def batch(cuda):
    """1,030 rays of 128 samples (bump weights), on the device."""
    z, w, rows = make_inputs(1030, 128, 'bump', seed=5)
    return tuple(torch.from_numpy(a).to(cuda) for a in (w, z, rows))


@pytest.mark.parametrize('lindisp', [False, True])
def test_loss_only_launch_and_halves_are_bit_equal(lindisp, batch):
    w, z, rows = batch
    L, g = kernel(w, z, rows, lindisp)
    L_only, none = kernel(w, z, rows, lindisp, want_grad=False)
    assert none is None
    np.testing.assert_array_equal(bits(L_only), bits(L))
    parts = [kernel(w[s].contiguous(), z[s].contiguous(), rows[s].contiguous(), lindisp) for s in (slice(0, 500), slice(500, None))]
    np.testing.assert_array_equal(bits(torch.cat([p[0] for p in parts])), bits(L))
    np.testing.assert_array_equal(bits(torch.cat([p[1] for p in parts])), bits(g))
    # 8-column rows (no view directions) carry the same near / far: the same result
    L8, g8 = kernel(w, z, rows[:, :8].contiguous(), lindisp)
    np.testing.assert_array_equal(bits(L8), bits(L))
    np.testing.assert_array_equal(bits(g8), bits(g))


@pytest.mark.parametrize('S,at', [(192, 70), (64, 63), (65, 0)])
@pytest.mark.parametrize('what', ['weight', 'depth'])
def test_a_nan_poisons_its_own_ray_only(what, S, at, cuda):
    z, w, rows = (torch.from_numpy(a).to(cuda) for a in make_inputs(8, S, 'uniform', seed=S))
    L, g = kernel(w, z, rows, False)
    bad_w, bad_z = w.clone(), z.clone()
    (bad_w if what == 'weight' else bad_z)[3, at] = float('nan')
    Lb, gb = kernel(bad_w, bad_z, rows, False)
    assert not torch.isfinite(Lb[3]) and not torch.isfinite(gb[3]).any()
    keep = [0, 1, 2, 4, 5, 6, 7]
    np.testing.assert_array_equal(bits(Lb[keep]), bits(L[keep]))
    np.testing.assert_array_equal(bits(gb[keep]), bits(g[keep]))
    assert torch.isfinite(L).all() and torch.isfinite(g).all()


def test_autograd_returns_the_kernels_gradient(batch):
    w, z, rows = batch
    w = w[:300].contiguous()
    z, rows = z[:300].contiguous(), rows[:300].contiguous()
    L, g = kernel(w, z, rows, True)
    wr = w.clone().requires_grad_(True)
    out = ops.distortion_loss(wr, z, rows, lindisp=True)
    assert out.shape == (300,) and out.dtype == torch.float32 and out.requires_grad
    np.testing.assert_array_equal(bits(out), bits(L))
    got, = torch.autograd.grad(out.sum(), wr)
    np.testing.assert_array_equal(bits(got), bits(g))
    c = torch.linspace(-2., 3., 300, device=w.device)
    got_c, = torch.autograd.grad((ops.distortion_loss(wr, z, rows, lindisp=True) * c).sum(), wr)
    np.testing.assert_array_equal(bits(got_c), bits(c[:, None] * g))
    # no gradient asked for: the loss-only launch, the same loss; z and rows get none
    zr = z.clone().requires_grad_(True)
    plain = ops.distortion_loss(w, zr, rows, lindisp=True)
    assert not plain.requires_grad
    np.testing.assert_array_equal(bits(plain), bits(L))
    with torch.no_grad():
        np.testing.assert_array_equal(bits(ops.distortion_loss(wr, z, rows, lindisp=True)), bits(L))
    # a non-contiguous `weights` gives what its contiguous copy gives
    wide = torch.rand(300, 256, device=w.device)
    wide[:, ::2] = w
    nc = wide[:, ::2].requires_grad_(True)
    assert not nc.is_contiguous()
    out_nc = ops.distortion_loss(nc, z, rows, lindisp=True)
    got_nc, = torch.autograd.grad(out_nc.sum(), nc)
    np.testing.assert_array_equal(bits(out_nc), bits(L))
    np.testing.assert_array_equal(bits(got_nc), bits(g))


def test_empty_batch_and_refusals(batch, cuda):
    w, z, rows = (t[:4].contiguous() for t in batch)
    assert ops.distortion_loss(w[:0], z[:0], rows[:0]).shape == (0,)
    for bad in ((w[:, :5], z, rows), (w, z, rows[:3]), (w, z, rows[:, :9]), (w[0], z[0], rows), (w, z, rows[:, 6])):
        with pytest.raises(_lib.MvipError, match='distortion_loss'):
            ops.distortion_loss(*bad)
    with pytest.raises(_lib.MvipError, match='distortion_loss'):
        ops.distortion_loss(w.cpu(), z.cpu(), rows.cpu())
    with pytest.raises(_lib.MvipError, match='distortion_loss'):
        ops.distortion_loss(w, z.cpu(), rows)


# ---- render_rays(..., distortion=True) --------------------------------------------------------------------------------------

def bench_rows(cuda, B, seed=0):
    sel = torch.from_numpy(np.random.RandomState(seed).randint(0, bench.H * bench.W, B)).to(cuda)
    return ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)


@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8x256 pair with a density head that renders something (the construction of tests/test_occupancy.py,
    written again): alpha_linear rescaled to sigma' = 4 (sigma - median) / std over the camera's sample points."""
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    rows = bench_rows(cuda, 2000, seed=99)
    z = ops.stratified_z(rows, 64, True)
    pts = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rows[:, None, 8:11].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    for net, seed in ((te['network_fn'], 1), (te['network_fine'], 2)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        with torch.no_grad():
            sigma = net.query_points(pts, dirs)[:, 3]
            scale = 4.0 / float(sigma.std())
            net.alpha_linear.bias.copy_((net.alpha_linear.bias - sigma.median()) * scale)
            net.alpha_linear.weight.mul_(scale)
        net.invalidate_packed()
    return te


def render(te, rows, **kw):
    return run.render_rays(rows, te['network_fn'], te['network_query_fn'], 64, lindisp=True, N_importance=64,
                           network_fine=te['network_fine'], white_bkgd=True, **kw)


@pytest.mark.parametrize('grad', [True, False], ids=['grad', 'no_grad'])
def test_render_rays_keys_are_the_op_on_the_calls_own_outputs(grad, mlp, cuda):
    rows = bench_rows(cuda, 37, seed=37)
    with torch.set_grad_enabled(grad):
        torch.manual_seed(0)
        ref = render(mlp, rows, retraw=True, need_alpha=True)
        torch.manual_seed(0)
        got = render(mlp, rows, retraw=True, need_alpha=True, distortion=True)
        assert 'dist_loss' not in ref and 'dist_loss0' not in ref                # the default adds no key
        d1, d0 = got.pop('dist_loss'), got.pop('dist_loss0')
        assert sorted(got) == sorted(ref)
        for k in ref:                                                            # every other key: the call without the keyword
            assert got[k].dtype == ref[k].dtype
            np.testing.assert_array_equal(N(got[k]), N(ref[k]), err_msg=k)
        assert d1.shape == d0.shape == (37,) and d1.dtype == d0.dtype == torch.float32
        assert d1.requires_grad == d0.requires_grad == grad
        np.testing.assert_array_equal(bits(d1), bits(ops.distortion_loss(got['weights'], got['z_vals'], rows, lindisp=True)))
        # the coarse pass, rebuilt from existing ops
        z0 = ops.stratified_z(rows, 64, True, None)
        w0 = ops.composite(mlp['network_fn'].query_rays(rows, z0), z0, rows, None, True, False, False)[3]
        np.testing.assert_array_equal(bits(d0), bits(ops.distortion_loss(w0, z0, rows, lindisp=True)))
        z1 = ops.sample_pdf_merge(z0, w0, _uniforms((37,), 64, True, False, cuda))[1]
        np.testing.assert_array_equal(bits(z1), bits(got['z_vals']))
    d1, d0 = d1.detach(), d0.detach()
    assert torch.isfinite(d1).all() and torch.isfinite(d0).all() and float(d1.min()) > 0 and float(d0.min()) > 0
    assert float(d1.max()) < 1 and float(d0.max()) < 1                           # weights sum to at most 1 over a unit interval


def test_render_rays_gradients_reach_the_networks_the_weights_come_from(mlp, cuda):
    rows = bench_rows(cuda, 37, seed=38)
    coarse, fine = mlp['network_fn'], mlp['network_fine']

    def grads(**kw):
        for p in list(coarse.parameters()) + list(fine.parameters()):
            p.grad = None
        ret = render(mlp, rows, distortion=True, **kw)
        return ret

    ret = grads(coarse_grad=False)
    assert ret['dist_loss'].requires_grad and not ret['dist_loss0'].requires_grad
    ret['dist_loss'].sum().backward()
    assert all(p.grad is None for p in coarse.parameters())
    got = {k: p.grad for k, p in fine.named_parameters() if p.grad is not None}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for k in ('alpha_linear.weight', 'alpha_linear.bias', 'pts_linears.0.weight', 'pts_linears.7.weight'):   # the density path
        assert float(got[k].abs().sum()) > 0, k
    ret = grads()
    assert ret['dist_loss0'].requires_grad
    ret['dist_loss0'].sum().backward()
    assert all(p.grad is None or not bool(p.grad.any()) for p in fine.parameters())
    got = {k: p.grad for k, p in coarse.named_parameters() if p.grad is not None}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got['alpha_linear.weight'].abs().sum()) > 0 and float(got['pts_linears.0.weight'].abs().sum()) > 0
    for p in list(coarse.parameters()) + list(fine.parameters()):
        p.grad = None
    # render / batchify_rays pass the keyword through; chunks do not change the value
    H, W = 12, 16
    kw = dict(mlp, near=bench.NEAR, far=bench.FAR, distortion=True)
    with torch.no_grad():
        a = run.render(H, W, bench.FOCAL * W / bench.W, chunk=50, c2w=bench.orbit_pose(0, cuda), **kw)[4]
        b = run.render(H, W, bench.FOCAL * W / bench.W, chunk=H * W, c2w=bench.orbit_pose(0, cuda), **kw)[4]
    assert a['dist_loss'].shape == a['dist_loss0'].shape == (H, W)
    np.testing.assert_array_equal(bits(a['dist_loss']), bits(b['dist_loss']))
    np.testing.assert_array_equal(bits(a['dist_loss0']), bits(b['dist_loss0']))


# ---- trainer --------------------------------------------------------------------------------------------------------------

def trainer_args(**kw):
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3,
             basedir='/tmp/mvip_test', expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64,
             white_bkgd=True, raw_noise_std=0., dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False,
             N_rand=24, chunk=1 << 15, lrate_decay=10, depth_lambda=0.1, sds_loss_weight=1e-4, no_coarse=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_trainer_adds_the_weighted_term(cuda):
    from oracle.weights import seeded_state_dict
    from mvip_nerf_amd.trainer import SecondStageTrainer, SyntheticScene
    scene = SyntheticScene(H=20, W=28, focal=383.65 * 28 / 504, mask_hw=(6, 7), n_views=8, device=cuda)
    out = []
    for extra in ({}, {'distortion_lambda': 0.01}):
        torch.manual_seed(0)
        tr = SecondStageTrainer(trainer_args(**extra), scene, cuda, guidance=None)
        for net, seed in ((tr.kw_train['network_fn'], 51), (tr.kw_train['network_fine'], 52)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        assert tr.last_distortion is None
        loss, n_rays = tr.step(3)
        assert n_rays == 42 + 24 + 24
        out.append((float(loss), tr.last_distortion))
    (loss_0, none), (loss_l, term) = out
    assert none is None
    assert torch.is_tensor(term) and term.dim() == 0 and not term.requires_grad
    assert np.isfinite(float(term)) and float(term) > 0
    assert abs((loss_l - float(term)) - loss_0) <= 1e-6 * abs(loss_0), (loss_0, loss_l, float(term))
