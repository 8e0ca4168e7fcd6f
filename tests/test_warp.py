"""Reference-view propagation on the GPU (csrc/warp.hip, ops.warp_views, prepare.propagate_reference, the trainer's reference
term) against the restatement tests/warp_numpy.py.

The yardstick is the restatement in fp64 on the fp32 inputs.  Per case e32 = the restatement run in fp32 against it, computed
here; the GPU's colours and residuals agree with the fp64 run within 4 * e32 + 2^-22 (the factor 4 covers a different operation
order) and its index is equal, except on EXCLUDED pixels: those whose fp64 run has a decision within a margin (u or v within
2^-18 max(H, W) of 0 / W-1 / H-1, ||resid| - tol| < 2^-16, |t_s| < 2^-16).  At most 1 % of a case's masked pixels may be
excluded, which every case asserts; an excluded pixel must still hold a well-formed result.  Every test prints its figures.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_numpy as R                                   # noqa: E402

from mvip_nerf_amd import ops, prepare                   # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene1_small.npz')
_YARD = {}


def yardstick(name, args, **kw):
    """The restatement's figures of a case, computed once and left unchanged."""
    if name not in _YARD:
        _YARD[name] = R.yardstick(*args, **kw)
    return _YARD[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def gpu_warp(cuda, args, order=None, tol=0.05):
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in args[:6]]
    o = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(cuda)
    out = ops.warp_views(*t, args[6], order=o, tol=tol)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    assert all(not a.requires_grad and a.is_contiguous() for a in out)
    return tuple(a.cpu().numpy() for a in out)


def check(name, cuda, args, order=None, tol=0.05):
    """Run the case on the GPU and hold it to the yardstick; returns (gpu outputs, yardstick)."""
    y = yardstick(name, args, order=order, tol=tol)
    rgb, index, resid = gpu_warp(cuda, args, order, tol)
    mask = np.asarray(args[2]) != 0
    S = args[4].shape[0]
    excluded, keep = y['excluded'], mask & ~y['excluded']
    n_mask, n_ex = int(mask.sum()), int(excluded.sum())
    wrong = int((index != y['index'])[keep].sum())
    same = keep & (index == y['index'])
    err_rgb = float(np.abs(rgb.astype(np.float64) - y['rgb'])[same].max()) if same.any() else 0.0
    err_res = float(np.abs(resid.astype(np.float64) - y['resid'])[same].max()) if same.any() else 0.0
    b_rgb, b_res = 4.0 * y['e32_rgb'] + 2.0 ** -22, 4.0 * y['e32_resid'] + 2.0 ** -22
    print(f'{name}: masked {n_mask}, taken {int((y["index"] >= 0).sum())}, excluded {n_ex}, index differs on {wrong} kept pixels '
          f'(fp32 restatement: {y["index32_differs"]}); colour error {err_rgb:.3e} (e32 {y["e32_rgb"]:.3e}, bound {b_rgb:.3e}); resid '
          f'error {err_res:.3e} (e32 {y["e32_resid"]:.3e}, bound {b_res:.3e})')
    assert n_ex <= 0.01 * n_mask
    assert wrong == 0
    assert err_rgb <= b_rgb and err_res <= b_res
    # well-formed everywhere: unmasked pixels and pixels without a source hold 0 / -1 / 0, an index names a source, a taken
    # pixel is finite and within tol
    assert ((index >= -1) & (index < max(S, 1))).all() and (index[~mask] == -1).all()
    none = index < 0
    assert not bits(rgb)[none].any() and not bits(resid)[none].any()
    assert np.isfinite(rgb[~none]).all() and (np.abs(resid[~none]) <= np.float32(tol)).all()
    return (rgb, index, resid), y


# ---- the trial scene, the homography, the identity -------------------------------------------------------------------------------

def test_trial_scene(cuda):
    c = R.trial_scene()
    (rgb, index, resid), y = check('trial', cuda, R.args_of(c))
    valid = index[0] >= 0
    hidden = R.hidden_from(c['tgt_points'], c['src_pose'][0][:, 3], **R.TRIAL_BOX)
    print(f'trial: valid {valid.mean():.4f}, hidden from the source {int(hidden.sum())}')
    assert abs(valid.mean() - 0.87) < 0.005
    assert hidden.sum() >= 40 and not (hidden & valid).any()
    assert y['excluded'].sum() == 0 and np.array_equal(index, y['index'])


def test_homography(cuda):
    c = R.homography_case()
    assert (c['H'], c['W']) == (33, 47)
    (rgb, index, resid), y = check('homography', cuda, R.args_of(c))
    taken = index[0] >= 0
    # the disparity of a plane is affine in the pixel coordinates, so its bilinear read is exact: the residual is rounding
    assert taken.sum() >= 0.9 * c['tgt_mask'].sum() and np.abs(resid[0][taken]).max() <= 4.0 * y['e32_resid'] + 2.0 ** -22 + 1e-6


def test_identity_interior(cuda):
    c = R.homography_case()                                  # the source warped onto itself: every border pixel is on the threshold
    args = (c['src_disp'], c['src_pose'], c['tgt_mask'], c['src_rgb'], c['src_disp'], c['src_pose'], c['focal'])
    (rgb, index, resid), y = check('identity', cuda, args)
    m = c['tgt_mask'][0]
    assert (index[0][m] == 0).all() and np.abs(rgb[0] - c['src_rgb'][0])[m].max() <= 4.0 * y['e32_rgb'] + 2.0 ** -22 + 1e-6


# ---- degenerate inputs: every one gives -1 ------------------------------------------------------------------------------------------

def degenerate(kind):
    c = R.homography_case()
    a = {k: np.array(c[k]) for k in R.ARGS[:6]}
    a['tgt_mask'][:] = True
    if kind == 'source_behind':                              # the source looks the other way: t_s < 0
        a['src_pose'][0] = R.pose((0.0, np.pi, 0.0), (-0.2, 0.1, 0.05))
    elif kind == 'target_looks_away':                        # the target's points lie to the side of and behind the source
        a['tgt_pose'][0] = R.pose((0.0, 2.0, 0.0), (0.1, -0.05, 0.0))
    elif kind == 'tgt_nan':
        a['tgt_disp'][:] = np.nan
    elif kind == 'tgt_zero':
        a['tgt_disp'][:] = 0.0
    elif kind == 'tgt_negative':
        a['tgt_disp'] *= -1.0
    elif kind == 'tgt_inf':
        a['tgt_disp'][:] = np.inf
    elif kind == 'src_nan':
        a['src_disp'][:] = np.nan
    elif kind == 'src_zero':
        a['src_disp'][:] = 0.0
    elif kind == 'src_negative':
        a['src_disp'] *= -1.0
    elif kind == 'colour_nan':
        a['src_rgb'][..., 1] = np.nan
    return tuple(a[k] for k in R.ARGS[:6]) + (c['focal'],)


@pytest.mark.parametrize('kind', ['source_behind', 'target_looks_away', 'tgt_nan', 'tgt_zero', 'tgt_negative', 'tgt_inf', 'src_nan',
                                  'src_zero', 'src_negative', 'colour_nan'])
def test_degenerate_inputs_give_no_source(kind, cuda):
    (rgb, index, resid), y = check('degenerate_' + kind, cuda, degenerate(kind))
    assert (index == -1).all() and (y['index'] == -1).all() and not rgb.any() and not resid.any()


def two_by_two(behind):
    f = 2.0
    tgt, src = R.pose((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), R.pose((0.0, np.pi if behind else 0.0, 0.0), (0.3, -0.2, 0.0))
    plane = ((0.0, 0.0, 1.0), -2.0)
    rgb = np.random.RandomState(4).rand(1, 2, 2, 3).astype(np.float32)
    return (R.plane_disparity(tgt, 2, 2, f, *plane).astype(np.float32)[None], tgt[None], np.ones((1, 2, 2), bool), rgb,
            R.plane_disparity(src, 2, 2, f, *plane).astype(np.float32)[None], src[None], f)


def test_smallest_image(cuda):
    (_, index, _), _ = check('2x2_behind', cuda, two_by_two(True))
    assert (index == -1).all()
    (_, index, _), _ = check('2x2', cuda, two_by_two(False))             # the same frame with the source turned round: taps at the size limit
    assert (index >= 0).sum() >= 1 and (index == -1).sum() >= 1


def test_single_bad_taps(cuda):
    """One NaN colour pixel and one NaN / one negative disparity pixel in the trial scene's source: the target pixels that tap
    them lose their source, the rest keeps it."""
    c = R.trial_scene()
    clean = yardstick('trial', R.args_of(c))
    a = {k: np.array(c[k]) for k in R.ARGS[:6]}
    a['src_rgb'][0, 10, 30, 2] = np.nan
    a['src_disp'][0, 30, 12], a['src_disp'][0, 40, 50] = np.nan, -0.25
    (_, index, _), y = check('trial_bad_taps', cuda, tuple(a[k] for k in R.ARGS[:6]) + (c['focal'],))
    lost = (clean['index'] >= 0) & (index < 0)
    print('bad taps: pixels that lost their source', int(lost.sum()))
    assert 3 <= lost.sum() <= 3 * 9 and not ((clean['index'] < 0) & (index >= 0)).any()


# ---- the order of preference ------------------------------------------------------------------------------------------------------------

def test_preference_order(cuda):
    c = R.homography_case()
    H, W, f = c['H'], c['W'], c['focal']
    nrm, off = (0.15, -0.1, 1.0), -3.0
    srcs = [c['src_pose'][0], R.pose((0.02, 0.08, 0.0), (0.35, 0.0, 0.02)), R.pose((0.0, np.pi, 0.0), (0.0, 0.0, 0.0))]
    tgts = [c['tgt_pose'][0], R.pose((-0.02, 0.0, 0.02), (0.0, 0.1, 0.0))]
    disp = lambda p: R.plane_disparity(p, H, W, f, nrm, off).astype(np.float32)
    args = (np.stack([disp(p) for p in tgts]), np.stack(tgts), np.ones((2, H, W), bool),
            np.stack([R.smooth_image(H, W, 20 + k) for k in range(3)]), np.stack([disp(p) for p in srcs]), np.stack(srcs), f)
    order = np.array([[1, 0, 2], [5, -3, 0]], np.int32)
    (_, index, _), _ = check('preference', cuda, args, order=order)
    alone = [R.warp(*args, order=np.array([[k, -1, -1]] * 2, np.int32))[1] >= 0 for k in range(3)]
    both = alone[0][0] & alone[1][0]
    print(f'preference: target 0: source 1 passes on {int(alone[1][0].sum())}, source 0 on {int(alone[0][0].sum())}, both on {int(both.sum())}')
    assert both.sum() >= 500 and (alone[0][0] & ~alone[1][0]).sum() >= 20 and not alone[2].any()
    assert (index[0][alone[1][0]] == 1).all() and (index[0][alone[0][0] & ~alone[1][0]] == 0).all()
    assert (index[0][~alone[0][0] & ~alone[1][0]] == -1).all()
    assert (index[1][alone[0][1]] == 0).all() and (index[1][~alone[0][1]] == -1).all()      # 5 and -3 are skipped
    # order=None is the ascending order
    got = gpu_warp(cuda, args)
    asc = gpu_warp(cuda, args, order=np.array([[0, 1, 2]] * 2, np.int32))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, asc)) and (got[1][0][both] == 0).all()


# ---- empty inputs -----------------------------------------------------------------------------------------------------------------------

def test_empty_inputs(cuda):
    c = R.homography_case()
    args = list(R.args_of(c))
    args[2] = np.zeros_like(args[2])
    rgb, index, resid = gpu_warp(cuda, args)                 # empty mask
    assert not bits(rgb).any() and (index == -1).all() and not bits(resid).any()
    args = list(R.args_of(c))
    rgb, index, resid = gpu_warp(cuda, [args[0][:0], args[1][:0], args[2][:0]] + args[3:])      # N = 0
    assert rgb.shape == (0, 33, 47, 3) and index.shape == (0, 33, 47) and resid.shape == (0, 33, 47)
    rgb, index, resid = gpu_warp(cuda, args[:3] + [args[3][:0], args[4][:0], args[5][:0], args[6]])      # S = 0
    assert rgb.shape == (1, 33, 47, 3) and not bits(rgb).any() and (index == -1).all() and not bits(resid).any()
    rgb, index, resid = gpu_warp(cuda, args[:3] + [args[3][:0], args[4][:0], args[5][:0], args[6]], order=np.zeros((1, 0), np.int32))
    assert (index == -1).all()


# ---- the dataset's rasters: the bound, determinism -----------------------------------------------------------------------------------

def fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    img = z['images'].astype(np.float32) / np.float32(255.)
    disp = z['depths'].astype(np.float32) / np.float32(255.)
    P = z['poses']
    H, W = img.shape[1:3]
    return img, disp, z['masks'].astype(bool), np.ascontiguousarray(P[:, :, :4]), float(P[0, 2, 4]) * W / float(P[0, 1, 4])


def test_fixture_meets_the_bound(cuda):
    img, disp, masks, pose, focal = fixture()
    assert disp.shape == (30, 141, 252)
    (rgb, index, _), y = check('fixture', cuda, (disp, pose, np.ones_like(masks), img[:1], disp[:1], pose[:1], focal))
    cover = [float(((index[n] >= 0) & masks[n]).sum()) / float(masks[n].sum()) for n in (1, 5, 15, 29)]
    print('fixture: coverage inside the masks of views 1, 5, 15, 29:', ' '.join(f'{v:.3f}' for v in cover))
    assert all(abs(v - want) <= 0.5e-3 + 1e-9 for v, want in zip(cover, (0.986, 1.0, 0.985, 0.983)))


def test_batch_equals_single_calls_bit_for_bit(cuda):
    img, disp, masks, pose, focal = fixture()
    views, srcs = [1, 5, 15, 29], [0, 10, 20]
    order = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0], [2, 7, 1]], np.int32)
    m = np.ones((4,) + masks.shape[1:], bool)
    m[1] = masks[5]
    args = (disp[views], pose[views], m, img[srcs], disp[srcs], pose[srcs], focal)
    batch = gpu_warp(cuda, args, order=order)
    again = gpu_warp(cuda, args, order=order)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(batch, again))
    for n in range(4):
        one = gpu_warp(cuda, (args[0][n:n + 1], args[1][n:n + 1], args[2][n:n + 1]) + args[3:], order=order[n:n + 1])
        assert all(np.array_equal(bits(a[0]), bits(b[n])) for a, b in zip(one, batch)), n
    print('batch: sources taken per target', [np.bincount(batch[1][n][batch[1][n] >= 0], minlength=3).tolist() for n in range(4)])
    assert all(len(np.unique(batch[1][n])) >= 3 for n in (0, 2))


# ---- propagate_reference ------------------------------------------------------------------------------------------------------------

def test_propagate_reference(cuda):
    img, disp, masks, pose, focal = fixture()
    views = [0, 1, 5, 15, 20]
    img, disp, masks, pose = img[views], disp[views], masks[views], pose[views]
    refs = [0, 4]
    ref_images = np.stack([img[0], np.clip(img[4] * 0.5 + 0.25, 0, 1)]).astype(np.float32)      # view 20's reference differs from its image
    out = prepare.propagate_reference(img, masks, disp, pose, focal, refs, ref_images=ref_images)
    assert sorted(out) == ['coverage', 'holes', 'images', 'info', 'resid', 'source']
    got, source, holes = out['images'].cpu().numpy(), out['source'].cpu().numpy(), out['holes'].cpu().numpy()
    assert got.shape == img.shape and got.dtype == np.float32 and source.dtype == np.int32 and holes.dtype == bool
    others = [1, 2, 3]
    for n in others:                                         # unmasked pixels bit for bit
        assert np.array_equal(bits(got[n])[~masks[n]], bits(img[n])[~masks[n]])
    for k, v in enumerate(refs):                             # a reference view is returned unchanged
        assert np.array_equal(bits(got[v]), bits(ref_images[k])) and (source[v][masks[v]] == k).all() and (source[v][~masks[v]] == -1).all()
    assert np.array_equal(holes, masks & (source < 0)) and not holes[refs].any()
    # the warp inside: ops.warp_views over the masks with the references ordered by camera distance
    order = prepare.reference_order(pose, refs)
    assert order.shape == (5, 2) and order.dtype == np.int32 and sorted(order[2].tolist()) == [0, 1]
    dist = np.linalg.norm(pose[:, None, :, 3].astype(np.float64) - pose[refs][None, :, :, 3], axis=-1)
    assert all(dist[n, order[n, 0]] <= dist[n, order[n, 1]] for n in range(5))
    m = masks.copy()
    m[refs] = False
    rgb, index, resid = gpu_warp(cuda, (disp, pose, m, ref_images, disp[refs], pose[refs], focal), order=order)
    for n in others:
        assert np.array_equal(source[n], index[n]) and np.array_equal(bits(out['resid'].cpu().numpy()[n]), bits(resid[n]))
        taken = index[n] >= 0
        assert np.array_equal(bits(got[n])[taken], bits(rgb[n])[taken])
    cover = [float(((source[n] >= 0) & masks[n]).sum()) / float(masks[n].sum()) for n in range(5)]
    print('propagate_reference: coverage', [round(c, 4) for c in cover], 'holes', holes.sum((1, 2)).tolist(),
          'fill iterations', out['info']['iterations'].tolist())
    assert np.allclose(out['coverage'], cover, rtol=0, atol=1e-12) and out['coverage'][0] == 1.0 and holes.sum() > 0
    # the holes: ops.harmonic_fill per channel on the same inputs, bit for bit
    planes = torch.from_numpy(np.ascontiguousarray(got.transpose(0, 3, 1, 2).reshape(15, *masks.shape[1:]))).to(cuda)
    hole_planes = torch.from_numpy(np.ascontiguousarray(np.repeat(holes[:, None], 3, 1).reshape(15, *masks.shape[1:]))).to(cuda)
    want, info = ops.harmonic_fill(planes, hole_planes)
    want = want.cpu().numpy().reshape(5, 3, *masks.shape[1:]).transpose(0, 2, 3, 1)
    assert np.array_equal(bits(got)[holes], bits(want)[holes]) and np.array_equal(info['iterations'], out['info']['iterations'])
    assert info['converged'].all() and len(out['info']['unknowns']) == 15
    # fill=False leaves the images' own values in the holes
    raw = prepare.propagate_reference(img, masks, disp, pose, focal, refs, ref_images=ref_images, fill=False)
    r = raw['images'].cpu().numpy()
    assert raw['info'] is None and np.array_equal(bits(r)[~holes], bits(got)[~holes])
    assert np.array_equal(bits(r[others])[holes[others]], bits(img[others])[holes[others]])
    # an unconverged fill is named; tensors on the device are taken as they are
    t = lambda a: torch.from_numpy(a).to(cuda)
    with pytest.raises(RuntimeError, match='did not converge'):
        prepare.propagate_reference(t(img), t(masks), t(disp), t(pose), focal, refs, max_iters=1)
    loose = prepare.propagate_reference(t(img), t(masks), t(disp), t(pose), focal, refs, max_iters=1, allow_unconverged=True)
    assert not loose['info']['converged'].all()


# ---- trainer ----------------------------------------------------------------------------------------------------------------------------

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


def test_trainer_adds_the_reference_term(cuda):
    from oracle.weights import seeded_state_dict
    from mvip_nerf_amd.trainer import SecondStageTrainer, SyntheticScene
    lam, view = 0.5, 2
    scene = SyntheticScene(H=20, W=28, focal=383.65 * 28 / 504, mask_hw=(6, 7), n_views=8, device=cuda)
    idx = scene.masked_idx_of(view)
    half = torch.zeros((8, 20, 28), dtype=torch.bool, device=cuda)
    half.reshape(8, -1)[:, idx[::2]] = True
    out = {}
    for name, extra, valid in (('off', {}, None), ('on', {'reference_lambda': lam}, None),
                               ('none_valid', {'reference_lambda': lam}, torch.zeros_like(half)), ('half_valid', {'reference_lambda': lam}, half)):
        torch.manual_seed(0)
        scene.reference_valid = valid
        tr = SecondStageTrainer(trainer_args(**extra), scene, cuda, guidance=_ImagePrior())
        for net, seed in ((tr.kw_train['network_fn'], 51), (tr.kw_train['network_fine'], 52)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
            net.invalidate_packed()
        assert tr.last_reference is None
        # the term, independently: the masked render before the step (through the training kernels, as the step renders it)
        rgb = tr._render_pixels(scene.poses[view], idx, retraw=True, coarse_grad=False, **tr.kw_train)['rgb_map'].detach().double()
        sq = ((rgb - scene.images[view].reshape(-1, 3)[idx].double()) ** 2).cpu().numpy()
        loss, _ = tr.step(3, img_i=view)
        out[name] = (float(loss), tr.last_reference, sq)
    del scene.reference_valid
    loss_0, none, sq = out['off']
    assert none is None
    for name, want in (('on', lam * sq.mean()), ('none_valid', 0.0), ('half_valid', lam * sq[::2].mean())):
        loss_l, term, _ = out[name]
        assert torch.is_tensor(term) and term.dim() == 0 and not term.requires_grad
        print(f'trainer {name}: loss {loss_l:.8f} against {loss_0:.8f}, term {float(term):.8f}, independently {want:.8f}')
        assert abs(float(term) - want) <= 1e-6 * want
        assert abs((loss_l - loss_0) - want) <= 1e-6 * abs(loss_0), (loss_0, loss_l, want)
    assert float(out['none_valid'][1]) == 0.0
    assert out['on'][0] > loss_0 and float(out['on'][1]) > 0
