"""feature_linear folded into the view layer of the no-grad fp32 forward (NeRF.fold_feature_inference; csrc/mlp_fwd16_fold.hip,
mlp_fold_pack16_kernel) on the GPU: the packed tail, folded against unfolded kernels, the fused render, the untouched C
entries, cache refresh, and training left alone.  The algebra and its rounding bound are tests/test_fold_cpu.py."""
import types

import numpy as np
import pytest
import torch

from oracle.weights import seeded_state_dict, bench_like_rays
from test_fold_cpu import (fold_tail_numpy, PACKED_FLOATS, PACKED_FOLD_FLOATS, SEC_A_FLOATS, FOLD_TAIL_A)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6            # kernel against kernel, as tests/test_hip_kernels.py uses for the two-wave kernel


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def params_dev(seed, dev):
    from mvip_nerf_amd import ops
    sd = seeded_state_dict(int(seed))
    return [T(sd[k], dev) for k in ops.PARAM_ORDER]


def make_args(**kw):
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3,
             basedir='/tmp/mvip_test', expname='none', ft_path=None, no_reload=True, perturb=1., N_samples=64,
             white_bkgd=True, raw_noise_std=1., dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def build(seed_c, seed_f, dev, fold=True):
    from mvip_nerf_amd import run
    tr, te, _, grad_vars, opt = run.create_nerf(make_args(), device=dev)
    for net, seed in ((tr['network_fn'], seed_c), (tr['network_fine'], seed_f)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(int(seed)).items()})
        net.fold_feature_inference = fold
    return tr, te, grad_vars, opt


def render(te, rays, **kw):
    from mvip_nerf_amd import run
    with torch.no_grad():
        return run.render_rays(rays, te['network_fn'], te['network_query_fn'], 64, lindisp=True, perturb=0., raw_noise_std=0.,
                               white_bkgd=True, N_importance=64, network_fine=te['network_fine'], retraw=True, **kw)


def test_fold_pack_tail_is_exact(cuda):
    """The device pack against the numpy restatement: EXACT.  Both accumulate every element of W' and b' in fp64 over
    k = 0..255 in ascending order (fp32 x fp32 products are exact in fp64, so there is nothing a fused multiply-add could
    change) and round once.  The head of the extended image is the plain image, and repacking gives the same bits."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd._lib import ptr, stream, call
    assert ops.packed_floats() == PACKED_FLOATS and ops.packed_fold_floats() == PACKED_FOLD_FLOATS
    for seed in (1, 77):
        ps = params_dev(seed, cuda)
        packed = ops.mlp_pack(ps)
        img = ops.mlp_pack16(ps, packed)
        assert img.numel() == PACKED_FOLD_FLOATS
        plain = torch.empty(PACKED_FLOATS, device=cuda)
        call('mvip_mlp_pack16', _lib.ptr_array(ps), ptr(packed), ptr(plain), stream())
        assert torch.equal(bits(img[:PACKED_FLOATS]), bits(plain))
        want = fold_tail_numpy(seeded_state_dict(seed), N(plain[SEC_A_FLOATS:]))
        np.testing.assert_array_equal(N(img[FOLD_TAIL_A:]).view(np.int32), want.view(np.int32))
        lazy = ops.mlp_pack16(ps, packed, fold=False)
        ops.mlp_fold_pack16(ps, lazy)
        assert torch.equal(bits(lazy), bits(img))


def test_folded_kernel_against_unfolded(golden, cuda):
    """Folded and unfolded kernels from ONE extended image, points and rays, ragged sizes: sigma bit-equal (layers 0..7 and
    the sigma head run the same blocks in the same order), rgb within the kernel-vs-kernel tolerance, both within it of the
    golden forward; a part of the batch equals the same rows of the whole."""
    from mvip_nerf_amd import ops
    g = golden('mlp_fwd_bwd')
    ps = params_dev(g['seed'], cuda)
    packed = ops.mlp_pack(ps)
    img = ops.mlp_pack16(ps, packed)
    pts, dirs = T(g['pts'], cuda), T(g['dirs'], cuda)
    with torch.no_grad():
        fold = ops.mlp_points(pts, dirs, packed, ps, packed16=img)
        plain = ops.mlp_points(pts, dirs, packed, ps, packed16=ops.plain16(img))
    assert torch.equal(bits(fold[:, 3]), bits(plain[:, 3]))
    np.testing.assert_allclose(N(fold), N(plain), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(N(fold), g['out'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(N(plain), g['out'], rtol=RTOL, atol=ATOL)
    assert not torch.equal(bits(fold[:, :3]), bits(plain[:, :3]))     # the two really are different kernels
    for n_ in (1, 15, 17, 127, 129, 250):
        with torch.no_grad():
            pf = ops.mlp_points(pts[:n_].contiguous(), dirs[:n_].contiguous(), packed, ps, packed16=img)
            pp = ops.mlp_points(pts[:n_].contiguous(), dirs[:n_].contiguous(), packed, ps, packed16=ops.plain16(img))
        assert torch.equal(bits(pf), bits(fold[:n_])), n_
        assert torch.equal(bits(pp), bits(plain[:n_])), n_
    for B_ in (1, 15, 17, 127, 129, 250):
        rows = T(bench_like_rays(B_, seed=B_), cuda)
        z = ops.stratified_z(rows, 64, True)
        with torch.no_grad():
            rf = torch.full((B_, 64, 4), float('nan'), device=cuda)
            rf.copy_(ops.mlp_rays(rows, z, packed, ps, packed16=img))
            rp = ops.mlp_rays(rows, z, packed, ps, packed16=ops.plain16(img))
            p3 = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
            d3 = rows[:, None, 8:11].expand(B_, 64, 3).reshape(-1, 3)
            rf_pts = ops.mlp_points(p3, d3, packed, ps, packed16=img)
        assert torch.isfinite(rf).all(), B_
        assert torch.equal(bits(rf[..., 3]), bits(rp[..., 3])), B_
        np.testing.assert_allclose(N(rf), N(rp), rtol=RTOL, atol=ATOL, err_msg=str(B_))
        assert torch.equal(bits(rf.reshape(-1, 4)), bits(rf_pts)), B_      # rays and points forms of the folded kernel agree


def test_folded_kernel_propagates_non_finite(golden, cuda):
    """One point with a NaN and one with an infinite coordinate: their outputs are non-finite exactly as the unfolded kernel
    reports them (the NaN-preserving ReLU is unchanged), every other point is untouched."""
    from mvip_nerf_amd import ops
    g = golden('mlp_fwd_bwd')
    ps = params_dev(g['seed'], cuda)
    packed = ops.mlp_pack(ps)
    img = ops.mlp_pack16(ps, packed)
    pts, dirs = T(g['pts'], cuda).clone(), T(g['dirs'], cuda)
    with torch.no_grad():
        clean = ops.mlp_points(pts, dirs, packed, ps, packed16=img)
        pts[5, 1] = float('nan')
        pts[140, 0] = float('inf')
        fold = ops.mlp_points(pts, dirs, packed, ps, packed16=img)
        plain = ops.mlp_points(pts, dirs, packed, ps, packed16=ops.plain16(img))
    assert torch.isnan(fold[5]).all() and torch.isnan(plain[5]).all()
    assert torch.equal(torch.isfinite(fold), torch.isfinite(plain))
    assert torch.equal(torch.isnan(fold), torch.isnan(plain))
    assert not torch.isfinite(fold[140]).any()
    keep = torch.ones(pts.shape[0], dtype=torch.bool, device=cuda)
    keep[5] = keep[140] = False
    assert torch.equal(bits(fold[keep]), bits(clean[keep]))


@pytest.mark.parametrize('B', [96, 257])
def test_fused_render_with_fold(cuda, B):
    """Folded fused coarse + fine launches: bit-identical to the folded six-launch chain, and within the golden tolerance
    of tests/test_render.py (rtol 1e-4, atol 1e-5 on rgb_map) of the unfolded render."""
    from mvip_nerf_amd import run
    rays = T(bench_like_rays(B, seed=B), cuda)
    _, te, _, _ = build(31, 32, cuda, fold=True)
    fused = render(te, rays, need_alpha=True)
    run.FUSED_RENDER = False
    try:
        chain = render(te, rays, need_alpha=True)
    finally:
        run.FUSED_RENDER = True
    assert set(fused) == set(chain)
    for k in fused:
        assert torch.equal(bits(fused[k]), bits(chain[k])), k
    _, te_off, _, _ = build(31, 32, cuda, fold=False)
    plain = render(te_off, rays, need_alpha=True)
    np.testing.assert_allclose(N(fused['rgb_map']), N(plain['rgb_map']), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(fused['acc_map']), N(plain['acc_map']), rtol=1e-4, atol=1e-5)
    assert not torch.equal(bits(fused['raw'][..., :3]), bits(plain['raw'][..., :3]))
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        render(te, rays)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if e.device_time_total > 0 and 'mlp_forward16_kernel' in e.key]
    assert len(names) == 2, names          # the coarse and the fine instantiation, no fold pack (the image is cached)
    assert not any('fold_pack' in e.key for e in prof.key_averages())


def test_plain_c_entries_still_run_the_unfolded_network(golden, cuda):
    """mvip_mlp_pack16 / forward_rays16 / forward_points16 / render_*_fused on a plain 597,248-float image, called through
    the C boundary: same bits as the unfolded route through ops (which hands them the head of the extended image)."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd._lib import ptr, stream, call
    g = golden('mlp_fwd_bwd')
    ps = params_dev(g['seed'], cuda)
    packed = ops.mlp_pack(ps)
    plain = torch.empty(PACKED_FLOATS, device=cuda)
    call('mvip_mlp_pack16', _lib.ptr_array(ps), ptr(packed), ptr(plain), stream())
    img = ops.mlp_pack16(ps, packed)
    pts, dirs = T(g['pts'], cuda), T(g['dirs'], cuda)
    raw = torch.empty(256, 4, device=cuda)
    call('mvip_mlp_forward_points16', ptr(plain), ptr(pts), ptr(dirs), 256, ptr(raw), stream())
    np.testing.assert_allclose(N(raw), g['out'], rtol=RTOL, atol=ATOL)
    with torch.no_grad():
        assert torch.equal(bits(raw), bits(ops.mlp_points(pts, dirs, packed, ps, packed16=ops.plain16(img))))
    B = 37
    rows = T(bench_like_rays(B, seed=3), cuda)
    z = ops.stratified_z(rows, 64, True)
    raw_r = torch.empty(B, 64, 4, device=cuda)
    call('mvip_mlp_forward_rays16', ptr(plain), ptr(rows), ptr(z), B, 64, ptr(raw_r), stream())
    with torch.no_grad():
        assert torch.equal(bits(raw_r), bits(ops.mlp_rays(rows, z, packed, ps, packed16=ops.plain16(img))))
        u = torch.linspace(0., 1., 64, device=cuda)
        c_plain = ops.render_coarse_fused(plain, rows, True, None, None, u, True)
        c_head = ops.render_coarse_fused(ops.plain16(img), rows, True, None, None, u, True)
        c_fold = ops.render_coarse_fused(img, rows, True, None, None, u, True)
        zm = c_plain[4]
        f_plain = ops.render_fine_fused(plain, rows, zm, None, True, want_raw=True)
        f_head = ops.render_fine_fused(ops.plain16(img), rows, zm, None, True, want_raw=True)
        f_fold = ops.render_fine_fused(img, rows, zm, None, True, want_raw=True)
    for a_, b_ in zip(c_plain + f_plain, c_head + f_head):
        assert (a_ is None and b_ is None) or torch.equal(bits(a_), bits(b_))
    np.testing.assert_allclose(N(c_fold[0]), N(c_plain[0]), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(f_fold[0]), N(f_plain[0]), rtol=1e-4, atol=1e-5)
    assert torch.equal(bits(f_fold[6][..., 3]), bits(f_plain[6][..., 3]))          # sigma of the fine pass: same bits
    with pytest.raises(_lib.MvipError):
        ops.render_fine_fused(img[:1000], rows, zm, None, True)


def test_parameter_update_refreshes_folded_tail(cuda):
    """The folded tail follows the weights: optimizer.step() (version counters) and an in-place .data write followed by
    invalidate_packed() both give what a fresh module with the same weights renders."""
    rays = T(bench_like_rays(64, seed=9), cuda)
    tr, te, grad_vars, opt = build(41, 42, cuda)
    first = render(te, rays)
    fine = tr['network_fine']

    def fresh_like():
        tr2, te2, _, _ = build(41, 42, cuda)
        for a_, b_ in ((tr2['network_fn'], tr['network_fn']), (tr2['network_fine'], fine)):
            a_.load_state_dict({k: v.detach().clone() for k, v in b_.state_dict().items()})
        return render(te2, rays)

    # 1: an optimizer step on feature_linear.weight alone
    sgd = torch.optim.SGD([fine.feature_linear.weight], lr=0.05)
    fine.feature_linear.weight.grad = torch.ones_like(fine.feature_linear.weight) * torch.linspace(
        -1., 1., 256, device=cuda)[:, None]
    sgd.step()
    second = render(te, rays)
    assert not torch.equal(bits(second['rgb_map']), bits(first['rgb_map']))
    assert torch.equal(bits(second['raw'][..., 3]), bits(first['raw'][..., 3]))      # sigma does not see feature_linear
    want = fresh_like()
    for k in second:
        assert torch.equal(bits(second[k]), bits(want[k])), k
    # 2: a write through .data (no version bump), then invalidate_packed()
    fine.feature_linear.weight.data.mul_(0.5)
    fine.feature_linear.bias.data.add_(0.25)
    stale = render(te, rays)
    assert torch.equal(bits(stale['rgb_map']), bits(second['rgb_map']))              # documented: .data writes need the call
    fine.invalidate_packed()
    third = render(te, rays)
    assert not torch.equal(bits(third['rgb_map']), bits(second['rgb_map']))
    want = fresh_like()
    for k in third:
        assert torch.equal(bits(third[k]), bits(want[k])), k


def test_training_step_does_not_see_the_fold(cuda):
    """A training step after a no-grad render does not depend on the fold:
      * everything its forward produces (every output of the training render, the loss) is bit-identical with folding on
        and off -- the stash-writing forward reads the head of the image;
      * with the folded tail of both cached images overwritten by NaN after the no-grad render, the step still gives the same
        bits and finite gradients: the training path never reads the tail;
      * a training-only iteration of a new weight version launches the plain pack but no fold pack.
    The parameter gradients themselves are accumulated with fp32 atomics (include/mvip_nerf.h, mvip_mlp_backward_*), so their
    bits differ from run to run with ANY setting (the test prints whether two runs with folding off agree); they are
    compared with the rel-L2 bound 1e-5 per tensor, two orders above the reordering noise of fp32 sums of this length and
    three below the bound tests/test_hip_kernels.py uses between the one- and two-wave training forwards (1e-2)."""
    from mvip_nerf_amd import run
    rays = T(bench_like_rays(48, seed=4), cuda)
    target = torch.rand(48, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    kw = dict(lindisp=True, perturb=0., raw_noise_std=0., white_bkgd=True, N_importance=64, retraw=True)
    results = {}
    for tag, fold, poison in (('on', True, False), ('on_poisoned', True, True), ('off', False, False), ('off_again', False, False)):
        tr, te, grad_vars, opt = build(51, 52, cuda, fold=fold)
        render(te, rays)
        if poison:
            for net in (tr['network_fn'], tr['network_fine']):
                assert net._packed_w16.numel() == PACKED_FOLD_FLOATS and net._packed_w16_folded
                net._packed_w16[PACKED_FLOATS:] = float('nan')
        r = run.render_rays(rays, tr['network_fn'], tr['network_query_fn'], 64, network_fine=tr['network_fine'], **kw)
        loss = ((r['rgb_map'] - target) ** 2).mean() + ((r['rgb0'] - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        grads = [p.grad.detach().clone() for p in grad_vars]
        assert all(torch.isfinite(g_).all() for g_ in grads), tag
        opt.step()
        results[tag] = ({k: v.detach().clone() for k, v in r.items()}, loss.detach().clone(), grads)
        if tag == 'on':
            # a training-only iteration of the NEW weight version packs the plain images but not the folded tail
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                r2 = run.render_rays(rays, tr['network_fn'], tr['network_query_fn'], 64, network_fine=tr['network_fine'], **kw)
                r2['rgb_map'].sum().backward()
                torch.cuda.synchronize()
            keys = [e.key for e in prof.key_averages()]
            assert any('mlp_pack16_kernel' in k for k in keys), keys
            assert not any('fold_pack' in k for k in keys), keys
            assert not tr['network_fine']._packed_w16_folded
    ref_out, ref_loss, ref_grads = results['off']
    same_setting = all(torch.equal(bits(a_), bits(b_)) for a_, b_ in zip(ref_grads, results['off_again'][2]))
    print('gradients of two runs with folding off bit-identical:', same_setting)
    for tag in ('on', 'on_poisoned', 'off_again'):
        out, loss, grads = results[tag]
        assert set(out) == set(ref_out)
        for k in out:
            assert torch.equal(bits(out[k]), bits(ref_out[k])), (tag, k)
        assert torch.equal(bits(loss), bits(ref_loss)), tag
        for a_, b_ in zip(grads, ref_grads):
            assert float((a_ - b_).norm()) <= 1e-5 * float(b_.norm()), tag
