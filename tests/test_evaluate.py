"""mvip_nerf_amd/evaluate.py on the GPU: image_metrics on the scene fixture, evaluate_views with a seeded model at 24 x 32,
evaluate_folders on PNGs written by prepare.write_images."""
import os
import types

import numpy as np
import pytest
import torch

from mvip_nerf_amd import evaluate, ops, prepare, run
from mvip_nerf_amd.run_nerf_helpers import img2l1, img2mse, mse2psnr

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene1_small.npz')


def fixture_pair(cuda, views=(0, 1)):
    z = np.load(FIXTURE, allow_pickle=False)
    img = torch.from_numpy(z['images'][list(views)].astype(np.float32) / np.float32(255.)).to(cuda)
    return img[:, :, 1:].contiguous(), img[:, :, :-1].contiguous(), torch.from_numpy(z['masks'][list(views)].astype(bool)).to(cuda)


def test_image_metrics_on_the_fixture(cuda):
    pred, gt, m = fixture_pair(cuda)
    mask = m[:, :, 1:].contiguous()
    plain = evaluate.image_metrics(pred, gt)
    assert sorted(plain) == ['l1', 'l2', 'psnr', 'ssim'] and all(len(v) == 2 for v in plain.values())
    out = evaluate.image_metrics(pred, gt, mask)
    assert sorted(out) == ['l1', 'l2', 'psnr', 'psnr_bbox', 'psnr_masked', 'ssim', 'ssim_bbox', 'ssim_masked']
    s, sm = ops.ssim(pred, gt).cpu().tolist(), ops.ssim(pred, gt, mask=mask).cpu().tolist()
    print('fixture:', {k: [round(v, 5) if v is not None else None for v in vs] for k, vs in out.items()})
    for n in range(2):
        assert out['psnr'][n] == float(mse2psnr(img2mse(pred[n], gt[n]))) == plain['psnr'][n]
        assert out['l2'][n] == float(img2mse(pred[n], gt[n])) and out['l1'][n] == float(img2l1(pred[n], gt[n]))
        assert out['ssim'][n] == s[n] == plain['ssim'][n] and out['ssim_masked'][n] == sm[n]
        y0, y1, x0, x1 = evaluate.mask_bbox(mask[n])
        assert y1 - y0 >= 11 and x1 - x0 >= 11
        p, g = pred[n:n + 1, y0:y1, x0:x1].contiguous(), gt[n:n + 1, y0:y1, x0:x1].contiguous()
        assert out['ssim_bbox'][n] == float(ops.ssim(p, g)) and out['psnr_bbox'][n] == float(mse2psnr(img2mse(p, g)))
        assert out['psnr_masked'][n] == float(mse2psnr(img2mse(pred[n][mask[n]], gt[n][mask[n]])))
        assert 0.0 < out['ssim'][n] < 1.0 and 5.0 < out['psnr'][n] < 60.0
    # a mask whose rectangle is 8 pixels wide: PSNR on the crop, no SSIM; an empty mask: nothing
    narrow = torch.zeros_like(mask)
    narrow[0, 30:60, 100:108] = True
    out = evaluate.image_metrics(pred, gt, narrow)
    assert out['ssim_bbox'] == [None, None] and out['psnr_bbox'][0] is not None and out['psnr_bbox'][1] is None
    assert out['psnr_masked'][1] is None and out['ssim_masked'][1] == 1.0 and 0.0 < out['ssim_masked'][0] < 1.0
    with pytest.raises(ValueError, match='image_metrics'):
        evaluate.image_metrics(pred, gt[:1])
    with pytest.raises(ValueError, match='mask'):
        evaluate.image_metrics(pred, gt, mask[:, :-1])


def trainer_args(**kw):
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3,
             basedir='/tmp/mvip_test', expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64,
             white_bkgd=True, raw_noise_std=0., dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False,
             N_rand=24, chunk=1 << 15, lrate_decay=10, depth_lambda=0.1, sds_loss_weight=1e-4, no_coarse=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_evaluate_views_with_a_seeded_model(cuda):
    from oracle.weights import seeded_state_dict
    from mvip_nerf_amd.trainer import SyntheticScene
    H, W = 24, 32
    scene = SyntheticScene(H=H, W=W, focal=383.65 * W / 504, mask_hw=(12, 13), n_views=3, device=cuda)
    _, kw, _, _, _ = run.create_nerf(trainer_args(), cuda)
    for net, seed in ((kw['network_fn'], 51), (kw['network_fine'], 52)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        net.invalidate_packed()
    kw = {k: v for k, v in kw.items() if k not in ('near', 'far')}
    hwf = (H, W, scene.focal)
    rep = evaluate.evaluate_views(kw, hwf, scene.poses, scene.images, scene.near, scene.far, masks=scene.masks, disparities=scene.depths)
    keys = ['depth_l1', 'depth_l2', 'l1', 'l2', 'psnr', 'psnr_bbox', 'psnr_masked', 'ssim', 'ssim_bbox', 'ssim_masked']
    assert rep['views'] == 3 and sorted(rep['per_view']) == keys and sorted(rep['mean']) == keys
    assert all(len(v) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in v) for v in rep['per_view'].values())
    for k in keys:
        assert abs(rep['mean'][k] - float(np.mean(rep['per_view'][k]))) <= 1e-12
    with torch.no_grad():
        for n in range(3):
            rgb, disp = run.render(H, W, scene.focal, chunk=1 << 15, c2w=scene.poses[n], near=scene.near, far=scene.far, **kw)[:2]
            assert rep['per_view']['psnr'][n] == float(mse2psnr(img2mse(rgb, scene.images[n])))
            assert rep['per_view']['depth_l2'][n] == float(img2mse(disp, scene.depths[n]))
    print('evaluate_views:', {k: round(v, 5) for k, v in rep['mean'].items()})
    plain = evaluate.evaluate_views(kw, hwf, scene.poses[:1], scene.images[:1], scene.near, scene.far)
    assert sorted(plain['per_view']) == ['l1', 'l2', 'psnr', 'ssim'] and plain['per_view']['psnr'][0] == rep['per_view']['psnr'][0]
    with pytest.raises(ValueError, match='images'):
        evaluate.evaluate_views(kw, hwf, scene.poses, scene.images[:2], scene.near, scene.far)


def test_evaluate_folders_reproduces_the_in_memory_metrics(cuda, tmp_path):
    pred, gt, m = fixture_pair(cuda, views=(0, 1, 2))
    pred, gt, mask = pred[:, :60, :80].contiguous(), gt[:, :60, :80].contiguous(), torch.zeros((3, 60, 80), dtype=torch.bool, device=cuda)
    mask[0, 10:40, 20:50] = True
    mask[1, 5:25, 30:38] = True                              # 8 wide; view 2: empty
    names = ['view_b', 'view_a', 'view_c']                   # written out of order: paired by sorted name
    prepare.write_images(str(tmp_path / 'pred'), names, pred)
    prepare.write_images(str(tmp_path / 'gt'), names, gt)
    prepare.write_images(str(tmp_path / 'mask'), names, mask[..., None].expand(3, 60, 80, 3).float())
    d = lambda k: str(tmp_path / k / 'RGB_inpainted')
    rep = evaluate.evaluate_folders(d('pred'), d('gt'), d('mask'), device=cuda)
    assert rep['names'] == ['view_a', 'view_b', 'view_c'] and rep['views'] == 3
    order = [1, 0, 2]
    # the 8-bit images, quantised and divided on the host as the loader does (a division by a scalar on the device is a
    # multiplication by its reciprocal there, one ulp away)
    q = lambda t: torch.from_numpy(np.round(np.clip(t.cpu().numpy().astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8).astype(np.float32)
                                   / np.float32(255.)).to(cuda)
    want = evaluate.image_metrics(q(pred)[order], q(gt)[order], mask[order].contiguous())
    assert sorted(rep['per_view']) == sorted(want)
    for k, v in want.items():
        assert rep['per_view'][k] == v, k
    assert rep['per_view']['ssim_bbox'][0] is None and rep['per_view']['ssim_bbox'][1] is not None and rep['per_view']['psnr_masked'][2] is None
    path = evaluate.write_report(str(tmp_path / 'report.json'), rep)
    assert evaluate.read_report(path) == rep
    plain = evaluate.evaluate_folders(d('pred'), d('gt'), device=cuda)
    assert sorted(plain['per_view']) == ['l1', 'l2', 'psnr', 'ssim'] and plain['per_view']['ssim'] == rep['per_view']['ssim']
    os.remove(os.path.join(d('gt'), 'view_c.png'))
    with pytest.raises(ValueError, match='without a partner'):
        evaluate.evaluate_folders(d('pred'), d('gt'), device=cuda)
