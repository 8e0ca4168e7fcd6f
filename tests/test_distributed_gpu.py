"""Two-rank run of the real SecondStageTrainer on the GPU box (gloo transport, both ranks on GPU 0):
the sharded iteration -- strided ray shards, all_gather of the masked colours for the image-space
prior, one flat gradient all_reduce -- must reproduce the single-process gradients."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _args(full=False):
    return types.SimpleNamespace(
        is_normal_guidance=full, is_colla_guidance=full, normalmap_render_factor=2,
        multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
        netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3, basedir='/tmp/x',
        expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64, white_bkgd=True, raw_noise_std=0.,
        dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False, N_rand=32, chunk=1 << 15, lrate_decay=10,
        depth_lambda=0.1, sds_loss_weight=1e-2, no_coarse=False)


class _ImagePrior:
    """Stand-in for Pretrain_Model: a deterministic image-space loss on the ASSEMBLED frame, so a
    wrong gather order or a missing shard gradient shows up."""
    guidance = {}

    def cal_loss(self, i, a, b, c, combin_rgb, d, mask, e, B=1):
        H, W = combin_rgb.shape[-2:]
        yy = torch.linspace(0, 1, H, device=combin_rgb.device)[:, None]
        xx = torch.linspace(0, 1, W, device=combin_rgb.device)[None, :]
        wgt = (1 + yy + 2 * xx)[None, None]
        loss = ((combin_rgb * wgt) ** 2).sum() * 1e-2
        if b is not None:                              # normal map [1,3,H_r,W_r] (configs[2])
            loss = loss + (b * torch.flip(b, [2]).detach() * 3.0).sum() * 1e-2
        if a is not None:                              # neighbour views [V,3,H_r,W_r] + masks [V,1,H,W] (configs[3]); as in
            # train_step_colla_sds only the last view carries gradient, the others enter as constants
            assert e.shape == (a.shape[0], 1, H, W)
            k = torch.arange(1, a.shape[0] + 1, device=a.device, dtype=a.dtype)[:, None, None, None]
            loss = loss + ((a[-1:] * k[-1:]) ** 2).sum() * 1e-2 + (a[:-1].detach() * a[-1:]).sum() * 1e-2
        return loss


def _run(rank, world, port, out, full=False):
    from mvip_nerf_amd.trainer import SecondStageTrainer, SyntheticScene
    from oracle.weights import seeded_state_dict
    dev = torch.device('cuda', 0)
    d = None
    if world > 1:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        d = dist
    try:
        scene = SyntheticScene(H=20, W=28, focal=383.65 * 28 / 504, mask_hw=(7, 9), n_views=8, device=dev)
        tr = SecondStageTrainer(_args(full), scene, dev, guidance=_ImagePrior(), world=world, rank=rank, dist=d)
        for net, seed in ((tr.kw_train['network_fn'], 61), (tr.kw_train['network_fine'], 62)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        tr.optimizer.step = lambda: None
        loss, n = tr.step(5)
        torch.save({'grads': [p.grad.detach().cpu() for p in tr.grad_vars], 'rays': n}, os.path.join(out, f'w{world}r{rank}.pt'))
    finally:
        if world > 1:
            dist.destroy_process_group()


def test_two_rank_trainer_equals_single(tmp_path, cuda):
    _run(0, 1, 0, str(tmp_path))
    mp.spawn(_run, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ref = torch.load(os.path.join(str(tmp_path), 'w1r0.pt'))
    a, b = (torch.load(os.path.join(str(tmp_path), f'w2r{r}.pt')) for r in (0, 1))
    assert a['rays'] + b['rays'] == ref['rays'] == 63 + 32 + 32
    for ga, gb, gr in zip(a['grads'], b['grads'], ref['grads']):
        assert torch.equal(ga, gb)                                   # identical after the all-reduce
        tol = 2e-3 * float(gr.abs().max()) + 1e-12
        np.testing.assert_allclose(ga.numpy(), gr.numpy(), rtol=2e-3, atol=tol)


def test_two_rank_trainer_full_guidance(tmp_path, cuda):
    """configs[2]/[3] branches of the iteration: reduced-resolution depth -> normal map, and the <=5 neighbour
    views, both ray-sharded and re-assembled by all_gather, must give the single-process gradients."""
    _run(0, 1, 0, str(tmp_path), True)
    mp.spawn(_run, args=(2, _free_port(), str(tmp_path), True), nprocs=2, join=True)
    ref = torch.load(os.path.join(str(tmp_path), 'w1r0.pt'))
    a, b = (torch.load(os.path.join(str(tmp_path), f'w2r{r}.pt')) for r in (0, 1))
    assert a['rays'] + b['rays'] == ref['rays'] == 63 + 32 + 32 + 140 + 140        # rays rendered WITH grad
    for ga, gb, gr in zip(a['grads'], b['grads'], ref['grads']):
        assert torch.equal(ga, gb)
        tol = 2e-3 * float(gr.abs().max()) + 1e-12
        np.testing.assert_allclose(ga.numpy(), gr.numpy(), rtol=2e-3, atol=tol)


# ---- SDS terms owned by different ranks (sds_shard) through the REAL StableDiffusion wrapper -------------------------
class _RecordingDist:
    """torch.distributed with every collective the trainer issues written down as (name, element count, dtype): a rank that
    skips or reorders one shows up as a different sequence (and, on hardware, as a hang)."""
    NAMES = ('all_reduce', 'all_gather', 'all_gather_into_tensor', 'broadcast', 'reduce_scatter', 'barrier', 'all_to_all')

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        f = getattr(dist, name)
        if name not in self.NAMES:
            return f

        def wrapped(*a, **k):
            t = next((x for x in a if torch.is_tensor(x)), None)
            if t is None and a and isinstance(a[0], (list, tuple)) and a[0] and torch.is_tensor(a[0][0]):
                t = a[0][0]
            self._log.append((name, None if t is None else int(t.numel()), None if t is None else str(t.dtype)))
            return f(*a, **k)
        return wrapped


def _run_view_sharded(rank, world, port, out, n_rand=16):
    """configs[3]-shaped iteration (RGB + normal + collaborative SDS) on a small LLFFScene, the stand-in diffusion
    networks behind the real wrapper; every SDS term is evaluated by exactly one rank."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    from mvip_nerf_amd.nerf.utils import Pretrain_Model
    from mvip_nerf_amd.scene import LLFFScene
    from mvip_nerf_amd.trainer import SecondStageTrainer
    from oracle.sds_standin import TinyVAE, TinyUNet, TinyScheduler, prompt_embedding
    from oracle.weights import seeded_state_dict
    dev = torch.device('cuda', 0)
    d = None
    collectives = []
    if world > 1:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        d = _RecordingDist(collectives)
    try:
        g = dict(np.load(os.path.join(os.path.dirname(__file__), 'golden', 'trainer_two_steps.npz')))
        scene = LLFFScene(g['images'], g['poses'], g['bds'], g['masks'], g['inpainted_depths'], device=dev, build_sets=False)
        cache = {}

        def encode_prompt(p, cfg):
            if (p, cfg) not in cache:
                cache[(p, cfg)] = prompt_embedding(p, cfg).to(dev)
            return cache[(p, cfg)]
        nets = types.SimpleNamespace(vae=TinyVAE().to(dev), unet=TinyUNet().to(dev), encode_prompt=encode_prompt,
                                     alphas_cumprod=TinyScheduler().alphas_cumprod)
        sd = StableDiffusion(dev, False, False, networks=nets)
        calls = []
        for name in ('image_grad', 'colla_view_share', 'colla_last_view_image_grad'):
            f = getattr(sd, name)
            setattr(sd, name, (lambda f, name: (lambda *a, **k: (calls.append(name), f(*a, **k))[1]))(f, name))
        opt = types.SimpleNamespace(is_rgb_guidance=True, is_colla_guidance=True, is_normal_guidance=True, text='a stone bench',
                                    text_normal='a normal map', rgb_guidance_scale=7.5, colla_guidance_scale=7.5,
                                    normal_guidance_scale=1.5, normal_start=0, lambda_guidance=1, uniform_sphere_rate=0)
        a = _args(True)
        a.N_rand, a.sds_loss_weight = n_rand, 1e-2
        tr = SecondStageTrainer(a, scene, dev, guidance=Pretrain_Model(opt, dev, {'SD': sd}), world=world, rank=rank, dist=d,
                                view_shard=True)
        for net, seed in ((tr.kw_train['network_fn'], 63), (tr.kw_train['network_fine'], 64)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        tr.optimizer.step = lambda: None
        rec = (torch.from_numpy(g['clf_batches'][0][:n_rand]).to(dev), torch.from_numpy(g['inp_batches'][0][:n_rand]).to(dev))
        loss, n = tr.step(2, img_i=1, records=rec)
        torch.save({'grads': [p.grad.detach().cpu() for p in tr.grad_vars], 'rays': n, 'calls': calls, 'collectives': collectives},
                   os.path.join(out, f'v{world}r{rank}.pt'))
    finally:
        if world > 1:
            dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_view_sharded_sds_equals_single_process(tmp_path, cuda, world):
    """north_star: "SDS views shard".  Every rank renders its ray shards, evaluates only the SDS terms it owns
    (RGB, normal, the neighbour views) and receives the others' image-space gradients: parameter gradients equal the
    single-process ones, and across the ranks each term ran exactly once."""
    _run_view_sharded(0, 1, 0, str(tmp_path))
    mp.spawn(_run_view_sharded, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ref = torch.load(os.path.join(str(tmp_path), 'v1r0.pt'))
    parts = [torch.load(os.path.join(str(tmp_path), f'v{world}r{r}.pt')) for r in range(world)]
    assert sorted(ref['calls']) == ['colla_last_view_image_grad', 'colla_view_share', 'colla_view_share', 'image_grad', 'image_grad']
    assert sorted(sum((p['calls'] for p in parts), [])) == sorted(ref['calls'])
    assert all(len(p['calls']) <= -(-5 // world) for p in parts)                  # round-robin ownership
    assert sum(p['rays'] for p in parts) == ref['rays']
    for k, gr in enumerate(ref['grads']):
        for p in parts[1:]:
            assert torch.equal(parts[0]['grads'][k], p['grads'][k])              # identical after the all-reduce
        tol = 3e-3 * float(gr.abs().max()) + 1e-12
        np.testing.assert_allclose(parts[0]['grads'][k].numpy(), gr.numpy(), rtol=3e-3, atol=tol)


@pytest.mark.slow
def test_eight_ranks_issue_one_collective_sequence(tmp_path, cuda):
    """VERDICT r5 task 6: the first real 8-GPU run must not hang.  The configs[3] iteration on EIGHT ranks (gloo, one device):
    7 SDS terms over 8 ranks (rank 7 owns none), 4 colour / depth rays over 8 ranks (ranks 4-7 hold EMPTY shards, so their
    graphs never complete the coarse gradient bucket inside backward) -- every rank must issue the SAME sequence of
    collectives (name, element count, dtype), the gradients must agree on all ranks and equal the single-process ones.
    Replaces the reference's nn.DataParallel scatter / gather (DS_NeRF/run.py:1491, :1527)."""
    world = 8
    _run_view_sharded(0, 1, 0, str(tmp_path), 4)
    mp.spawn(_run_view_sharded, args=(world, _free_port(), str(tmp_path), 4), nprocs=world, join=True)
    ref = torch.load(os.path.join(str(tmp_path), 'v1r0.pt'))
    parts = [torch.load(os.path.join(str(tmp_path), f'v{world}r{r}.pt')) for r in range(world)]
    seq0 = parts[0]['collectives']
    assert len(seq0) >= 6, seq0
    for r, p in enumerate(parts[1:], 1):
        assert p['collectives'] == seq0, (r, p['collectives'], seq0)
    assert sorted(sum((p['calls'] for p in parts), [])) == sorted(ref['calls'])       # every term exactly once across the node
    assert all(len(p['calls']) <= 1 for p in parts)
    assert sum(p['rays'] for p in parts) == ref['rays']
    for k, gr in enumerate(ref['grads']):
        for p in parts[1:]:
            assert torch.equal(parts[0]['grads'][k], p['grads'][k])
        tol = 3e-3 * float(gr.abs().max()) + 1e-12
        np.testing.assert_allclose(parts[0]['grads'][k].numpy(), gr.numpy(), rtol=3e-3, atol=tol)
    print('collective sequence of one configs[3] iteration on 8 ranks:', seq0)


# ---- the strong-scaling render: one frame over all ranks (bench.py --gpus N headline, run.render_sharded) -------------
def _run_sharded_render(rank, world, port, out):
    from mvip_nerf_amd import run
    from oracle.weights import seeded_state_dict
    import bench
    dev = torch.device('cuda', 0)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        tr, te, _, _, _ = run.create_nerf(bench.make_args(), device=dev)
        for net, seed in ((te['network_fn'], 71), (te['network_fine'], 72)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        H, W, focal = 37, 53, 383.65 * 53 / 504                      # 1,961 rays: ragged blocks for 2 and 3 ranks
        with torch.no_grad():
            maps = run.render_sharded(H, W, focal, bench.orbit_pose(3, dev), rank, world, dist, chunk=512, near=bench.NEAR,
                                      far=bench.FAR, **te)
            whole = run.render(H, W, focal, chunk=512, c2w=bench.orbit_pose(3, dev), near=bench.NEAR, far=bench.FAR, **te) if rank == 0 else None
        torch.save({'maps': [m.cpu() for m in maps], 'whole': None if whole is None else [m.cpu() for m in whole[:4]]},
                   os.path.join(out, f's{world}r{rank}.pt'))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_frame_render_equals_whole_frame(tmp_path, cuda, world):
    """run.render_sharded through the real kernels: every rank renders its contiguous block of the frame's rays, ONE
    all_gather assembles (rgb, disp, acc, depth) on every rank -- bit for bit the maps of render() on one device (rays are
    independent and the kernels chunk-invariant), on all ranks, for ragged block sizes."""
    mp.spawn(_run_sharded_render, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), f's{world}r{r}.pt')) for r in range(world)]
    whole = parts[0]['whole']
    assert tuple(whole[0].shape) == (37, 53, 3)
    for p in parts:
        for got, want in zip(p['maps'], whole):
            assert got.shape == want.shape
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


class _CollectingDist:
    """Stand-in process group for ONE process: all_gather hands back this rank's own block (the other blocks zero), so the
    caller can assemble the frame from the blocks of successive calls."""

    def get_backend(self):
        return 'gloo'

    def all_gather(self, parts, pad):
        for p in parts:
            p.zero_()
        parts[self.rank].copy_(pad)


def test_sharded_frame_render_general_row_assembly(cuda):
    """run.render_sharded with render()'s own defaults (ndc=True, use_viewdirs=False), and with a static camera, builds its ray
    rows the way render() does (DS_NeRF/run.py:1182-1207) instead of silently rendering the non-NDC view-direction frame
    (ADVICE r4): the blocks of three ranks, put together, equal render()'s maps bit for bit."""
    from mvip_nerf_amd import run
    from mvip_nerf_amd.dist_utils import block_bounds
    from oracle.weights import seeded_state_dict
    import bench
    dev = torch.device('cuda', 0)
    tr, te, _, _, _ = run.create_nerf(bench.make_args(), device=dev)
    for net, seed in ((te['network_fn'], 71), (te['network_fine'], 72)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
    H, W, focal = 21, 29, 383.65 * 29 / 504
    kw = {k: v for k, v in te.items() if k not in ('ndc', 'use_viewdirs')}
    c2w = bench.orbit_pose(3, dev)
    cases = [dict(ndc=False, use_viewdirs=True, c2w_staticcam=bench.orbit_pose(5, dev)[:3, :4]),     # static camera: general assembly
             dict(ndc=False, use_viewdirs=True)]                                                    # the one-launch row builder
    world = 3
    d = _CollectingDist()
    with torch.no_grad():
        for case in cases:
            whole = run.render(H, W, focal, chunk=256, c2w=c2w, near=bench.NEAR, far=bench.FAR, **case, **kw)[:4]
            got = [torch.zeros_like(m) for m in whole]
            for rank in range(world):
                d.rank = rank
                maps = run.render_sharded(H, W, focal, c2w, rank, world, d, chunk=256, near=bench.NEAR, far=bench.FAR, **case, **kw)
                lo, hi = block_bounds(H * W, rank, world)
                for g_, m in zip(got, maps):
                    g_.reshape(H * W, -1)[lo:hi] = m.reshape(H * W, -1)[lo:hi]
            for g_, w_ in zip(got, whole):
                assert torch.equal(g_.view(torch.int32), w_.view(torch.int32)), case.keys()
        # render()'s defaults (NDC rays, no view directions) need a network without a view branch on this path: the row
        # assembly alone is compared
        rays_o, rays_d = run.ops.get_rays(H, W, focal, c2w)
        rows_all = run._assemble_rows_general(H, W, focal, rays_o, rays_d, True, 0., 1., False, None, None)
        seen = {}
        real = run.batchify_rays

        def capture(rows, chunk, **kwargs):
            seen['rows'] = rows.clone()
            z = rows.new_zeros(rows.shape[0])
            return {'rgb_map': rows.new_zeros(rows.shape[0], 3), 'disp_map': z, 'acc_map': z, 'depth_map': z}
        run.batchify_rays = capture
        try:
            d.rank = 1
            run.render_sharded(H, W, focal, c2w, 1, world, d, chunk=256)              # ndc=True, near=0, far=1, no viewdirs
        finally:
            run.batchify_rays = real
        lo, hi = block_bounds(H * W, 1, world)
        assert seen['rows'].shape == (hi - lo, 8) and torch.equal(seen['rows'], rows_all[lo:hi])


@pytest.mark.slow
def test_bench_two_ranks_on_one_device_reports_strong_scaling(cuda):
    """`bench.py --gpus 2 --full` end to end on the GPU box: it starts its own two ranks (both on GPU 0 over gloo,
    MVIP_BENCH_SINGLE_DEVICE=1 -- the boxes have one GPU), renders the frame in two ray blocks joined by one all_gather, runs
    the sharded training legs, and prints ONE line whose `value` is the strong-scaling figure with the weak one beside it."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MVIP_BENCH_SINGLE_DEVICE='1', MVIP_GRAPHS_WITH_DIST='1', MASTER_ADDR='127.0.0.1')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '1', '--full', '--train-steps', '1',
                        '--sds-steps', '1', '--no-hashgrid', '--no-cpu-baseline'], cwd=root, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong' and d['steps'] == 1
    assert d['value'] > 0 and d['weak_rays_per_sec'] > 0 and d['value_1_same_run'] > 0
    # both ranks time-share ONE device here: the line must say so and claim no scaling efficiency for it
    assert d['ranks_share_one_device'] is True and d['strong_efficiency'] is None
    assert d['multi_gpu']['rccl_world'] == 2
    assert d['metric'].startswith('rays_per_sec') and d['unit'] == 'rays/s'
    # round 6 (VERDICT r5 task 1): every leg says which arithmetic it ran in; configs[2] / [3] carry BOTH, the f32 one on top
    assert d['dtype'] == 'f32'
    for leg in ('train', 'train_f16x3', 'train_with_sds', 'train_with_sds_f16x3', 'render_f16x3', 'sds'):
        assert 'dtype' in d[leg], leg
    for leg in ('config2_rgb_normal_sds', 'config3_rgb_normal_colla_sds'):
        assert d[leg]['f32']['dtype'].startswith('f32') and d[leg]['f16x3']['dtype'].startswith('f16x3')
        assert d[leg]['ms_per_step'] == d[leg]['f32']['ms_per_step'] and d[leg]['dtype'] == d[leg]['f32']['dtype']
        assert d[leg]['f16x3']['ms_per_step'] < d[leg]['f32']['ms_per_step']
    mg = d['multi_gpu']
    assert 'f32' in mg['predicted']['dtype'] and 'f16x3' in mg['predicted_f16x3']['dtype'] and 'sds_mode' in mg['predicted']
