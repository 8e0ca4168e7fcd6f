"""The trainer's D-SSIM reference term (args.reference_ssim_lambda): off by default, lambda * mean(1 - SSIM) of the assembled frame
against the scene's image inside the view's mask when on.  Built the way the reference-term test of tests/test_warp.py builds its
trainer.  (The weight-gradient flush is not bit-reproducible, so no parameters are compared.)"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_numpy as R                                   # noqa: E402

from mvip_nerf_amd import ops                            # noqa: E402

pytestmark = pytest.mark.gpu


class _ImagePrior:
    """Stand-in for the diffusion prior: a deterministic image-space loss on the assembled frame."""
    guidance = {}

    def cal_loss(self, i, a, b, c, combin_rgb, d, mask, e, B=1):
        return (combin_rgb ** 2).sum() * 1e-2


def trainer_args(**kw):
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3,
             basedir='/tmp/mvip_test', expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64,
             white_bkgd=True, raw_noise_std=0., dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False,
             N_rand=24, chunk=1 << 15, lrate_decay=10, depth_lambda=0.1, sds_loss_weight=1e-4, no_coarse=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def make_trainer(scene, cuda, **extra):
    from oracle.weights import seeded_state_dict
    from mvip_nerf_amd.trainer import SecondStageTrainer
    torch.manual_seed(0)
    tr = SecondStageTrainer(trainer_args(**extra), scene, cuda, guidance=_ImagePrior())
    for net, seed in ((tr.kw_train['network_fn'], 51), (tr.kw_train['network_fine'], 52)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        net.invalidate_packed()
    return tr


def frame_of(tr, scene, view, grad=False):
    """The frame the step assembles: the scene's image with the masked render written in (through the training kernels)."""
    idx = scene.masked_idx_of(view)
    with torch.set_grad_enabled(grad):
        rgb = tr._render_pixels(scene.poses[view], idx, retraw=True, coarse_grad=False, **tr.kw_train)['rgb_map']
    combin = scene.images[view].detach().clone().reshape(-1, 3).index_put((idx,), rgb).reshape(1, scene.H, scene.W, 3)
    return combin.contiguous(), rgb


def test_trainer_adds_the_ssim_term(cuda, monkeypatch):
    from mvip_nerf_amd.trainer import SyntheticScene
    lam, view = 0.5, 2
    scene = SyntheticScene(H=20, W=28, focal=383.65 * 28 / 504, mask_hw=(6, 7), n_views=8, device=cuda)
    calls = []
    real = ops.ssim
    monkeypatch.setattr(ops, 'ssim', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    mask = scene.mask_of(view).reshape(1, 20, 28)
    target = scene.images[view].reshape(1, 20, 28, 3).contiguous()
    out = {}
    for name, extra, valid in (('absent', {}, None), ('zero', {'reference_ssim_lambda': 0.0}, None),
                               ('on', {'reference_ssim_lambda': lam}, None),
                               ('none_valid', {'reference_ssim_lambda': lam}, torch.zeros((8, 20, 28), dtype=torch.bool, device=cuda))):
        scene.reference_valid = valid
        tr = make_trainer(scene, cuda, **extra)
        assert tr.last_reference_ssim is None
        frame, _ = frame_of(tr, scene, view)
        before = len(calls)
        loss, _ = tr.step(3, img_i=view)
        out[name] = (float(loss), tr.last_reference_ssim, frame, len(calls) - before)
    del scene.reference_valid
    loss_0 = out['absent'][0]
    for name in ('absent', 'zero'):
        assert out[name][1] is None and out[name][3] == 0              # off: the term is None and ops.ssim is not called
    assert abs(out['zero'][0] - loss_0) <= 1e-6 * abs(loss_0)
    # on: lambda (1 - ssim) of the same frame, by the op and by the fp64 restatement
    loss_l, term, frame, n_calls = out['on']
    assert n_calls == 1 and torch.is_tensor(term) and term.dim() == 0 and not term.requires_grad
    want = lam * (1.0 - float(real(frame, target, mask=mask.contiguous())))
    s64, _, count = R.ssim(frame.cpu().numpy(), target.cpu().numpy(), mask.cpu().numpy())
    print(f'trainer: loss {loss_l:.8f} against {loss_0:.8f}, term {float(term):.8f}, independently {want:.8f}, fp64 restatement '
          f'{lam * (1.0 - float(s64[0])):.8f}, counted {int(count[0])}')
    assert count[0] == 42
    assert abs(float(term) - want) <= 1e-6 * want and abs(want - lam * (1.0 - float(s64[0]))) <= 1e-5
    assert abs((loss_l - loss_0) - want) <= 1e-6 * abs(loss_0), (loss_0, loss_l, want)
    assert want > 0.05 and loss_l > loss_0
    # reference_valid all false: exactly zero
    loss_n, term, _, n_calls = out['none_valid']
    assert n_calls == 1 and float(term) == 0.0 and abs(loss_n - loss_0) <= 1e-6 * abs(loss_0)


def test_the_term_alone_reaches_the_masked_render(cuda):
    from mvip_nerf_amd.trainer import SyntheticScene
    view = 1
    scene = SyntheticScene(H=20, W=28, focal=383.65 * 28 / 504, mask_hw=(6, 7), n_views=8, device=cuda)
    tr = make_trainer(scene, cuda, reference_ssim_lambda=0.5)
    frame, rgb = frame_of(tr, scene, view, grad=True)
    rgb.retain_grad()
    term = 0.5 * (1.0 - ops.ssim(frame, scene.images[view].reshape(1, 20, 28, 3).contiguous(),
                                 mask=scene.mask_of(view).reshape(1, 20, 28).contiguous())).mean()
    term.backward()
    g = rgb.grad
    grads = [p.grad for p in tr.grad_vars if p.grad is not None]
    print(f'term {float(term.detach()):.6f}: gradient on the masked render up to {float(g.abs().max()):.3e}, {len(grads)} parameters reached, '
          f'largest {max(float(p.abs().max()) for p in grads):.3e}')
    assert tuple(g.shape) == (42, 3) and torch.isfinite(g).all() and (g != 0).all()
    assert grads and max(float(p.abs().max()) for p in grads) > 0


def test_small_frame_is_refused(cuda):
    from mvip_nerf_amd.trainer import SyntheticScene
    scene = SyntheticScene(H=10, W=28, focal=383.65 * 28 / 504, mask_hw=(4, 5), n_views=4, device=cuda)
    tr = make_trainer(scene, cuda, reference_ssim_lambda=0.5)
    with pytest.raises(ValueError, match='reference_ssim_lambda'):
        tr.step(0, img_i=1)
