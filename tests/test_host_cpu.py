"""CPU tests of host-side logic that needs no kernel launch: module construction, state-dict keys,
checkpoint format round trip (with and without the reference's `module.` prefix), PNG writer."""
import os
import types
import zlib

import numpy as np
import pytest
import torch


def make_args(tmp):
    return types.SimpleNamespace(
        multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
        netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3, basedir=str(tmp),
        expname='exp', ft_path=None, no_reload=False, perturb=1., N_samples=64, white_bkgd=True, raw_noise_std=1.,
        dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False)


def test_checkpoint_round_trip_with_module_prefix(tmp_path):
    from mvip_nerf_amd import run
    os.makedirs(tmp_path / 'exp')
    args = make_args(tmp_path)
    tr, te, start, grad_vars, opt = run.create_nerf(args, device=torch.device('cpu'))
    assert start == 0
    with torch.no_grad():
        for k, p in enumerate(grad_vars):
            p.fill_(0.001 * (k + 1))
    run.save_checkpoint(str(tmp_path / 'exp' / '000007.tar'), 7, tr, opt)
    ck = torch.load(str(tmp_path / 'exp' / '000007.tar'))
    assert set(ck) == {'global_step', 'network_fn_state_dict', 'network_fine_state_dict', 'optimizer_state_dict'}
    assert all(k.startswith('module.') for k in ck['network_fn_state_dict'])          # the reference's key form
    assert list(ck['network_fn_state_dict'])[0] == 'module.pts_linears.0.weight'
    tr2, _, start2, gv2, _ = run.create_nerf(args, device=torch.device('cpu'))         # auto-reload newest *.tar
    assert start2 == 7
    for a, b in zip(grad_vars, gv2):
        assert torch.equal(a, b)
    # and files written without the prefix load as well
    run.save_checkpoint(str(tmp_path / 'exp' / '000009.tar'), 9, tr, opt, module_prefix=False)
    assert run.create_nerf(args, device=torch.device('cpu'))[2] == 9


def test_nerf_module_matches_reference_layout():
    from mvip_nerf_amd.run_nerf_helpers import NeRF
    from mvip_nerf_amd import ops
    from oracle.weights import seeded_state_dict
    m = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    sd = seeded_state_dict(0)
    assert list(m.state_dict()) == list(sd)
    assert [tuple(v.shape) for v in m.state_dict().values()] == [v.shape for v in sd.values()]
    assert tuple(ops.PARAM_ORDER) == tuple(sd) and ops.PARAM_SHAPES == tuple(v.shape for v in sd.values())
    assert sum(p.numel() for p in m.parameters()) == 595844


def test_png_writer(tmp_path):
    from mvip_nerf_amd.run import _write_png
    img = (np.arange(5 * 7 * 3) % 256).astype(np.uint8).reshape(5, 7, 3)
    _write_png(str(tmp_path / 'a.png'), img)
    b = open(tmp_path / 'a.png', 'rb').read()
    assert b[:8] == b'\x89PNG\r\n\x1a\n' and b[12:16] == b'IHDR'
    i = b.index(b'IDAT')
    n = int.from_bytes(b[i - 4:i], 'big')
    raw = zlib.decompress(b[i + 4:i + 4 + n])
    rows = np.frombuffer(raw, np.uint8).reshape(5, 1 + 21)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(5, 7, 3), img)


def _stand_in_scene1_f4(root, src, g):
    """Scene 1's factor-4 folder rebuilt from tests/golden/llff_scene1_f4_src.npz: the real poses_bounds.npy and file
    names, and per view rasters of the real size whose integer sums equal the real ones (RGB bytes, label pixels, first
    depth channel), with the real values at the golden pixels.  Every output the reference's loader was recorded on
    (llff_scene1_f4.npz) is a function of exactly these, so the comparison below is the one made on the real scene."""
    from PIL import Image
    h, w, c = (int(v) for v in src['shape'])
    fixed = {int(a): (int(b), int(cc), np.round(px * 255).astype(np.int64)) for (a, b, cc), px in zip(g['pixel_idx'], g['pixels'])}

    def raster(total, shape, pins=()):
        flat = np.zeros(int(np.prod(shape)), np.int64)
        idx = [i for i, _ in pins]
        rest = total - sum(v for _, v in pins)
        free = flat.size - len(idx)
        q, r = divmod(rest, free)
        assert 0 <= q and q + (r > 0) <= 255
        free_mask = np.ones(flat.size, bool)
        free_mask[idx] = False
        fill = np.full(free, q, np.int64)
        fill[:r] += 1
        flat[free_mask] = fill
        for i, v in pins:
            flat[i] = v
        return flat.reshape(shape).astype(np.uint8)

    for sub in ('RGB_inpainted', 'label', 'Depth_inpainted'):
        os.makedirs(os.path.join(root, 'images_4', sub))
    np.save(os.path.join(root, 'poses_bounds.npy'), src['poses_bounds'])
    for v, name in enumerate(src['names']):
        pins = ()
        if v in fixed:
            b, cc, px = fixed[v]
            pins = [((b * w + cc) * c + k, int(px[k])) for k in range(c)]
        Image.fromarray(raster(int(src['rgb_sum'][v]), (h, w, c), pins)).save(os.path.join(root, 'images_4', 'RGB_inpainted', name))
        n_on, on = int(src['label_sum'][v]), int(src['label_max'][v])
        lab = np.zeros(h * w, np.uint8)
        lab[:n_on // on] = on
        assert (n_on // on) * on == n_on
        Image.fromarray(lab.reshape(h, w)).save(os.path.join(root, 'images_4', 'label', name))
        Image.fromarray(raster(int(src['depth_sum'][v]), (h, w))).save(os.path.join(root, 'images_4', 'Depth_inpainted', name))


def test_llff_loader_matches_reference(golden, tmp_path):
    """load_llff_data on the reference's own scene (factor 4) equals the reference loader's outputs
    (captured by oracle/gen_golden_llff.py).  The scene folder is a stand-in rebuilt from a 14 KB fixture
    (_stand_in_scene1_f4); the poses and bounds are the real file."""
    from mvip_nerf_amd.load_llff import load_llff_data
    g = golden('llff_scene1_f4')
    data = str(tmp_path / 'scene1')
    src = golden('llff_scene1_f4_src')
    _stand_in_scene1_f4(data, src, g)
    images, poses, bds, render_poses, i_test, masks, depths, mask_indices = load_llff_data(data, 4)
    assert tuple(images.shape) == tuple(g['images_shape']) and poses.shape == (60, 3, 5) and int(i_test) == int(g['i_test'])
    np.testing.assert_allclose(poses, g['poses'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bds, g['bds'], rtol=1e-6)
    np.testing.assert_allclose(render_poses, g['render_poses'], rtol=1e-5, atol=1e-6)
    # The recorded float32 means carry the float32 accumulation error of the recording (<= 4e-4 relative); the exact
    # per-view means of the real scene are the integer sums of the fixture.  The loader's rasters are checked against
    # the exact values, the recording against them as a cross-check of the two fixtures.
    n = images.shape[1] * images.shape[2]
    image_mean = src['rgb_sum'] / (n * 3 * 255.)
    depth_mean = src['depth_sum'] / (n * 255.)
    np.testing.assert_allclose(images.mean((1, 2, 3), dtype=np.float64), image_mean, rtol=1e-6)
    np.testing.assert_allclose(g['image_mean'], image_mean, rtol=1e-3)
    for (a, b, c), px in zip(g['pixel_idx'], g['pixels']):
        np.testing.assert_array_equal(images[a, b, c], px)
    np.testing.assert_allclose(masks.sum((1, 2)), g['mask_sum'], rtol=1e-6)
    np.testing.assert_allclose(depths.mean((1, 2), dtype=np.float64), depth_mean, rtol=1e-6)
    np.testing.assert_allclose(g['depth_mean'], depth_mean, rtol=1e-3)
    assert list(mask_indices) == list(g['mask_indices'])


def test_pose_processing_on_fixture_poses(golden):
    """process_poses is deterministic host math: spot-check invariants on the committed golden poses
    (runs everywhere): recentred average pose is the identity frame; hwf column preserved."""
    from mvip_nerf_amd.load_llff import poses_avg
    g = golden('llff_scene1_f4')
    hwf = g['poses'][0, :, 4]
    assert hwf[0] == 567 and hwf[1] == 1008 and abs(hwf[2] - 3069.17394 / 4) < 1e-2
    assert g['render_poses'].shape == (120, 3, 5)


@pytest.mark.parametrize('n', [2, 8])
def test_bench_launcher_spawns_ranks_itself(n):
    """`bench.py --gpus N --full` with no WORLD_SIZE starts N ranks before touching a GPU and relays ONE JSON line with
    n_gpus = N (launcher-only dry run over gloo; N = 8 is the full node the driver's scaling run uses); under an
    external launcher a mismatching --gpus fails loudly."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env['MVIP_BENCH_DRYRUN'] = '1'
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(n), '--steps', '1', '--warmup', '0', '--full'],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1 and json.loads(lines[0])['n_gpus'] == n
    rec = json.loads(lines[0])
    # the N > 1 headline is the STRONG-scaling form: the dry run passed a frame of ray rows through run.render_sharded
    # (contiguous blocks, one all_gather) on both ranks and says so
    assert rec['scaling'] == 'strong' and rec['sharded_frame_assembled'] is True and 'weak_rays_per_sec' in rec
    if n != 2:
        return
    bad = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '3'], env=dict(env, WORLD_SIZE='2', RANK='0'),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and 'WORLD_SIZE=2' in bad.stderr


@pytest.mark.parametrize('fault', ['HANG', 'RAISE'])
def test_bench_exit_status_reflects_a_failed_multi_rank_leg(fault):
    """A rank that hangs in (or raises before) a collective of the legs after the headline measurement: rank 0 still
    prints exactly ONE JSON line -- carrying `extra_legs_error` and what the process group really was -- and the
    launcher's exit status is NOT zero (a broken multi-GPU path once passed as a good scaling run with rc 0)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(MVIP_BENCH_DRYRUN='1', MVIP_BENCH_EXTRA_DEADLINE_S='6')
    env[f'MVIP_BENCH_DRYRUN_{fault}_RANK'] = '1'
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--full'],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and 'extra_legs_error' in rec and 'extra_leg' not in rec
    assert rec['multi_gpu'] == {'rccl_world': 2, 'backend': 'gloo'}
    # and the healthy run reports the same fields with status 0
    env.pop(f'MVIP_BENCH_DRYRUN_{fault}_RANK')
    ok = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--full'],
                        env=env, capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0, ok.stderr[-2000:]
    rec = json.loads([l for l in ok.stdout.splitlines() if l.startswith('{"metric"')][0])
    assert rec['extra_leg'] == 'done' and 'extra_legs_error' not in rec and rec['multi_gpu']['rccl_world'] == 2


def test_bench_dump_outputs_names_sample_and_size(tmp_path):
    """bench.dump_outputs on a frame-shaped render() result: the maps whole, the per-sample arrays on the same fixed ray
    sample (identical in every call), float32 only, within the 64 MB cap."""
    import torch
    import bench
    h, w, s = bench.H, bench.W, bench.N_SAMPLES + bench.N_IMPORTANCE
    g = torch.Generator().manual_seed(0)
    maps = [torch.rand(h, w, 3, generator=g)] + [torch.rand(h, w, generator=g) for _ in range(3)]
    extras = {'weights': torch.rand(h, w, s, generator=g), 'z_vals': torch.rand(h, w, s, generator=g),
              'rgb0': torch.rand(h, w, 3, generator=g), 'z_std': torch.rand(h, w, generator=g),
              'disp0': torch.rand(h, w, generator=g)}
    extras['disp0'][0, :3] = torch.tensor([float('nan'), float('inf'), -float('inf')])     # 0 / 0 rays give NaN disparity
    names = bench.dump_outputs(maps + [extras], str(tmp_path / 'a'))
    bench.dump_outputs(maps + [extras], str(tmp_path / 'b'))
    assert set(names) == set(bench.RENDER_OUTPUTS) | set(extras) | {'sample_ray_index', 'disp0_nonfinite'}
    total = 0
    for n in names:
        a, b = np.load(tmp_path / 'a' / f'{n}.npy'), np.load(tmp_path / 'b' / f'{n}.npy')
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), n
        total += a.nbytes
    d0, flag = np.load(tmp_path / 'a' / 'disp0.npy'), np.load(tmp_path / 'a' / 'disp0_nonfinite.npy')
    np.testing.assert_array_equal(d0[0, :3], 0)
    np.testing.assert_array_equal(flag[0, :3], [1, 2, 3])
    assert flag.sum() == 6 and np.array_equal(d0[flag == 0], extras['disp0'].numpy()[flag == 0])
    assert total <= bench.DUMP_MAX_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'rgb_map.npy'), maps[0].numpy())
    sel = np.load(tmp_path / 'a' / 'sample_ray_index.npy').astype(np.int64)
    assert len(sel) == bench.DUMP_SAMPLE_RAYS and (np.diff(sel) > 0).all()
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'weights.npy'), extras['weights'].reshape(h * w, s).numpy()[sel])


def test_clip_text_tower_matches_transformers(golden):
    """The prompt encoder body against the library class the reference instantiates (transformers' CLIPTextModel,
    seeded weights, fixture from oracle/gen_golden_clip.py): same key mapping, causal mask, quick-GELU, final norm."""
    import numpy as np
    import torch
    from mvip_nerf_amd.guidance.sd_nets import CLIPTextModel
    from oracle.weights import seeded_clip_text_state
    g = golden('clip_text')
    m = CLIPTextModel().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_clip_text_state(int(g['seed'])).items()})
    with torch.no_grad():
        out = m(torch.from_numpy(g['ids']))
    np.testing.assert_allclose(out.numpy(), g['last_hidden_state'], rtol=0, atol=2e-5 * float(np.abs(g['last_hidden_state']).max()))


def test_latent_distribution_and_timestep_embedding_host_paths():
    """guidance/sd_nets.py on the host (no device, no library): LatentDist forms diffusers' mean / logvar / std lazily and its
    scaled_sample is the pipeline's expression with autograd to the moments; timestep_sinusoid is diffusers'
    get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0)."""
    import math
    from mvip_nerf_amd.guidance import sd_nets
    g = torch.Generator().manual_seed(4)
    m = torch.randn(1, 8, 6, 5, generator=g).requires_grad_(True)
    noise = torch.randn(1, 4, 6, 5, generator=g)
    d = sd_nets.LatentDist(m)
    assert torch.equal(d.mean, m[:, :4]) and torch.equal(d.logvar, torch.clamp(m[:, 4:], -30.0, 20.0))
    assert torch.equal(d.std, torch.exp(0.5 * d.logvar))
    out = d.scaled_sample(noise, 0.18215)
    assert torch.equal(out, 0.18215 * (m[:, :4] + torch.exp(0.5 * torch.clamp(m[:, 4:], -30.0, 20.0)) * noise))
    out.sum().backward()
    assert m.grad is not None and float(m.grad[:, :4].min()) == pytest.approx(0.18215)
    t = torch.tensor([980.0, 3.0])
    emb = sd_nets.timestep_sinusoid(t, 320)
    k = torch.arange(160, dtype=torch.float32)
    args = t[:, None] * torch.exp(-math.log(10000.0) * k / 160)[None]
    assert emb.shape == (2, 320)
    assert torch.allclose(emb[:, :160], torch.cos(args), atol=1e-6) and torch.allclose(emb[:, 160:], torch.sin(args), atol=1e-6)


def test_scaling_model_predictions():
    """mvip_nerf_amd/scaling_model.py (VERDICT r4 task 4a): the per-leg time model bench.py emits as multi_gpu.predicted.
    Checked here: the collective formulas, the replay of sds_shard's ownership (configs[3]: 7 terms; at 8 ranks the critical
    path is one forward-only term + the term that waits for the latent sum), monotonic legs, and the hook in bench.py."""
    import json
    import bench
    from mvip_nerf_amd import scaling_model as sm
    c = dict(sm.DEFAULTS)
    bw = c['link_GBps'] * 1e9 * c['link_efficiency']
    assert sm.collective_ms('all_reduce', 8e6, 1) == 0.0
    assert abs(sm.collective_ms('all_reduce', 8e6, 8) - ((c['alpha_us'] + 14 * c['hop_us']) * 1e-3 + 2 * 7 / 8 * 8e6 / bw * 1e3)) < 1e-9
    assert abs(sm.collective_ms('all_gather', 8e6, 4) - ((c['alpha_us'] + 3 * c['hop_us']) * 1e-3 + 3 / 4 * 8e6 / bw * 1e3)) < 1e-9
    terms = sm.config_terms(3)
    assert len(terms) == 7 and sum(1 for p, _ in terms if p == 1) == 4
    t_full, t_fwd = 20.0, 15.0
    one = sm.sds_critical_path_ms(terms, 1, t_full, t_fwd, 0)
    assert abs(one - (4 * t_fwd + 3 * t_full)) < 1e-9                       # one GPU: back to back
    eight = sm.sds_critical_path_ms(terms, 8, t_full, t_fwd, 0)
    assert t_fwd + t_full < eight < t_fwd + t_full + 0.2                     # forward-only term, 64 KB all_reduce, the waiting term
    two = sm.sds_critical_path_ms(terms, 2, t_full, t_fwd, 0)
    assert abs(two - (2 * t_fwd + 2 * t_full)) < 0.2                         # rank 0: two latent terms, rgb, the last view
    m = {'frame_ms': 300.0, 'train_ms': 54.0, 'sds_ms': 21.0, 'config2_ms': 160.0, 'config3_ms': 440.0}
    p = sm.predict(m, fwd_share=0.775)
    for key in ('ms_per_step', 'train_ms', 'train_with_sds_ms', 'config2_ms', 'config3_ms'):
        vals = [p['N'][n][key] for n in (2, 4, 8)]
        assert vals[0] > vals[1] > vals[2] > 0, (key, vals)
    assert 0.97 < p['N'][8]['strong_efficiency'] < 1.0 and p['N'][8]['value'] > 7.5 * 378 * 504 / 0.3
    # the prior's terms do not shard below one term per rank: configs[1] cannot scale past ~3x, configs[3] past ~10x
    assert p['scaling_ceiling']['train_with_sds_ms']['max_speedup'] < 3.5 < p['scaling_ceiling']['config3_ms']['max_speedup']
    line = {'ms_per_step': 300.0, 'train': {'ms_per_step': 54.0}, 'sds': {'ms_per_step': 21.0},
            'config2_rgb_normal_sds': {'ms_per_step': 160.0}, 'config3_rgb_normal_colla_sds': {'ms_per_step': 440.0}}
    bench.add_scaling_prediction(line, 1)
    assert sorted(line['multi_gpu']['predicted']['N']) == [2, 4, 8]
    json.dumps(line)
    # round 6 (VERDICT r5 tasks 1 / 6): legs in both arithmetics -> two predictions, each on its own legs; the SDS step enters
    # in the mode the multi-rank legs will run it in (eager unless MVIP_GRAPHS_WITH_DIST=1), while the terms subtracted from
    # the ONE-GPU config legs are the graph replays those legs ran
    line = {'ms_per_step': 300.0, 'train': {'ms_per_step': 54.0}, 'train_f16x3': {'ms_per_step': 30.0}, 'render_f16x3': {'ms_per_step': 90.0},
            'sds': {'ms_per_step': 21.0, 'ms_per_step_eager': 22.5},
            'config2_rgb_normal_sds': {'ms_per_step': 280.0, 'f32': {'ms_per_step': 280.0}, 'f16x3': {'ms_per_step': 150.0}},
            'config3_rgb_normal_colla_sds': {'ms_per_step': 850.0, 'f32': {'ms_per_step': 850.0}, 'f16x3': {'ms_per_step': 400.0}}}
    old_env = os.environ.pop('MVIP_GRAPHS_WITH_DIST', None)
    try:
        bench.add_scaling_prediction(line, 1)
        pf, ps = line['multi_gpu']['predicted'], line['multi_gpu']['predicted_f16x3']
        assert pf['inputs']['sds_ms'] == 22.5 and pf['inputs']['sds_one_gpu_ms'] == 21.0 and 'eager' in pf['sds_mode']
        assert pf['inputs']['config2_ms'] == 280.0 and ps['inputs']['config2_ms'] == 150.0 and ps['inputs']['frame_ms'] == 90.0
        assert pf['N'][8]['config3_ms'] > ps['N'][8]['config3_ms'] > 0 and 'f32' in pf['dtype'] and 'f16x3' in ps['dtype']
        # the NeRF part isolated from a one-GPU leg does not depend on the multi-rank mode of the step
        direct = sm.predict({'frame_ms': 300.0, 'train_ms': 54.0, 'sds_ms': 21.0, 'config2_ms': 280.0, 'config3_ms': 850.0})
        assert pf['N'][8]['config2_ms'] > direct['N'][8]['config2_ms']           # eager terms on the critical path: slower than replays
        os.environ['MVIP_GRAPHS_WITH_DIST'] = '1'
        line.pop('multi_gpu')
        bench.add_scaling_prediction(line, 1)
        assert line['multi_gpu']['predicted']['inputs']['sds_ms'] == 21.0 and 'replay' in line['multi_gpu']['predicted']['sds_mode']
        assert abs(line['multi_gpu']['predicted']['N'][8]['config2_ms'] - direct['N'][8]['config2_ms']) < 1e-9
    finally:
        os.environ.pop('MVIP_GRAPHS_WITH_DIST', None)
        if old_env is not None:
            os.environ['MVIP_GRAPHS_WITH_DIST'] = old_env
    json.dumps(line)


def test_sd_checkpoint_manifest_and_strict_loading(tmp_path):
    """guidance/sd_checkpoint.py (VERDICT r4 task 9; the reference's from_pretrained + _encode_prompt,
    DS_NeRF/guidance/sd_utils.py:46-74, :317-326): the committed manifest equals what sd_nets builds (686 / 248 / 196 tensors, the
    published SD-1.5 counts), a synthetic diffusers-layout directory round-trips through safetensors AND .bin with transformers'
    / old-VAE key names, fp16-exactness is detected, and a wrong key set, a wrong shape or a missing file is refused."""
    import json
    import warnings
    from safetensors.torch import save_file
    from mvip_nerf_amd.guidance import sd_checkpoint as ck, sd_nets
    man = ck.manifest()
    assert {c: len(v) for c, v in man.items()} == {'unet': 686, 'vae': 248, 'text_encoder': 196}
    assert man == json.loads(json.dumps(ck.build_manifest()))          # committed fixture == the architecture as built
    assert man['unet']['conv_in.weight'] == [320, 9, 3, 3] and man['vae']['quant_conv.weight'] == [8, 8, 1, 1]
    assert man['text_encoder']['text_model.encoder.layers.11.mlp.fc1.weight'] == [3072, 768]
    # key maps are inverse to each other on every manifest key
    for comp in man:
        with torch.device('meta'):
            mod = {'unet': sd_nets.UNet2DConditionModel, 'vae': sd_nets.AutoencoderKL, 'text_encoder': sd_nets.CLIPTextModel}[comp]()
        assert {ck.map_key(comp, k) for k in man[comp]} == set(mod.state_dict())
    # ---- the VAE (the smallest network with old-name aliases) and the text tower, really written and read ----
    root = tmp_path / 'ckpt'
    g = torch.Generator().manual_seed(5)
    vae_src = sd_nets.AutoencoderKL()
    state = {}
    for k, v in vae_src.state_dict().items():
        v = (torch.randn(v.shape, generator=g) * 0.05).half().float()         # fp16-exact values, like revision="fp16" cast up
        state[k] = v
    old_names = {}
    for k, v in state.items():                                                  # write the attention block under its pre-0.15 names
        m = __import__('re').match(r'^(encoder|decoder)(\.mid_block\.attentions\.0\.)(to_q|to_k|to_v|to_out\.0)\.(weight|bias)$', k)
        if m:
            alias = {'to_q': 'query', 'to_k': 'key', 'to_v': 'value', 'to_out.0': 'proj_attn'}[m.group(3)]
            old_names[f'{m.group(1)}{m.group(2)}{alias}.{m.group(4)}'] = v
        else:
            old_names[k] = v
    os.makedirs(root / 'vae')
    save_file({k: v.half() for k, v in old_names.items()}, str(root / 'vae' / 'diffusion_pytorch_model.fp16.safetensors'))
    dst = sd_nets.AutoencoderKL()
    exact = ck.load_component(dst, 'vae', ck.find_weight_file(str(root), 'vae'))
    assert exact is True
    for k, v in dst.state_dict().items():
        assert torch.equal(v, state[k]), k
    # a tensor that is not an fp16 value -> three-product contractions
    bad = dict(old_names)
    bad['quant_conv.weight'] = bad['quant_conv.weight'] + 1e-5
    torch.save(bad, str(root / 'vae' / 'diffusion_pytorch_model.bin'))
    os.remove(root / 'vae' / 'diffusion_pytorch_model.fp16.safetensors')
    assert ck.load_component(sd_nets.AutoencoderKL(), 'vae', ck.find_weight_file(str(root), 'vae')) is False
    # wrong key set / wrong shape / missing file: refused, with the names
    miss = {k: v for k, v in old_names.items() if k != 'encoder.conv_in.bias'}
    miss['encoder.conv_in.extra'] = torch.zeros(3)
    torch.save(miss, str(root / 'vae' / 'diffusion_pytorch_model.bin'))
    with pytest.raises(ck.CheckpointError) as e:
        ck.load_component(sd_nets.AutoencoderKL(), 'vae', ck.find_weight_file(str(root), 'vae'))
    assert 'encoder.conv_in.bias' in str(e.value) and 'encoder.conv_in.extra' in str(e.value)
    shp = dict(old_names)
    shp['decoder.conv_out.weight'] = torch.zeros(3, 128, 1, 1)
    torch.save(shp, str(root / 'vae' / 'diffusion_pytorch_model.bin'))
    with pytest.raises(ck.CheckpointError, match='shapes'):
        ck.load_component(sd_nets.AutoencoderKL(), 'vae', ck.find_weight_file(str(root), 'vae'))
    with pytest.raises(ck.CheckpointError, match='none of'):
        ck.find_weight_file(str(root), 'unet')
    # text tower under transformers' names (+ the position_ids buffer of older files), read back into our module
    txt = sd_nets.CLIPTextModel(vocab=64, d=32, layers=2, heads=2, ctx=8)
    tstate = {ck.unmap_key('text_encoder', k): v.clone() for k, v in txt.state_dict().items()}
    assert 'text_model.encoder.layers.1.self_attn.q_proj.weight' in tstate and 'text_model.final_layer_norm.bias' in tstate
    tstate['text_model.embeddings.position_ids'] = torch.arange(8)[None]
    tiny_man = {'text_encoder': {k: list(v.shape) for k, v in tstate.items() if 'position_ids' not in k}}
    got = ck.check_against_manifest('text_encoder', tstate, tiny_man)
    assert set(got) == set(txt.state_dict())
    # tokenizer: the real BPE class when its files are there (a toy vocabulary), else the stand-in with a warning
    tdir = root / 'tokenizer'
    os.makedirs(tdir)
    vocab = {'<|startoftext|>': 0, '<|endoftext|>': 1, 'a</w>': 2, 'b</w>': 3, 'a': 4, 'b': 5, 'ab</w>': 6}
    json.dump(vocab, open(tdir / 'vocab.json', 'w'))
    open(tdir / 'merges.txt', 'w').write('#version: 0.2\na b</w>\n')
    tok = ck.CLIPBPETokenizer(str(tdir))
    ids = tok('ab a')
    assert ids.shape == (1, 77) and ids.dtype == torch.long and ids[0, 0] == 0 and ids[0, 1] == 6 and ids[0, 2] == 2 and ids[0, 3] == 1


def test_stable_diffusion_refuses_a_directory_that_is_not_a_checkpoint(tmp_path):
    """`StableDiffusion(device, fp16, vram_O, hf_key=<dir>)` (DS_NeRF/guidance/sd_utils.py:46) goes through the strict loader: an
    empty directory, or a hub NAME, raises instead of silently keeping random weights."""
    from mvip_nerf_amd.guidance import sd_checkpoint as ck

    class Nets:                                    # load_into touches nothing before the first file check
        unet = vae = text_encoder = None
        _cache = {}
    with pytest.raises(ck.CheckpointError, match='not a directory'):
        ck.load_into(Nets(), 'runwayml/stable-diffusion-inpainting')
    with pytest.raises(ck.CheckpointError, match='none of'):
        ck.load_into(Nets(), str(tmp_path))
