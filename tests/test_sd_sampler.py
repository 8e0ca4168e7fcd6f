"""The 2D sampler on the device: the decoder head kernel and the DDIM update kernel (csrc/sd_sample.hip) against fp64,
decode_latents against the same AutoencoderKL on the host, the launches of decode_latents, the graph-replayed denoising loop
against an explicit eager loop, and the public methods' determinism / shapes / step counts."""
import ctypes
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sd_network_cases import library_kernels_in                        # noqa: E402

pytestmark = pytest.mark.gpu

PROMPT = 'a stone bench in a park'


@pytest.fixture(scope='module')
def sd(cuda):
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    torch.manual_seed(0)
    s = StableDiffusion(cuda, False, False)
    assert s.use_graphs
    yield s
    s.release_graphs()


def _head_ref64(x, gamma, beta, w, b, G, eps):
    """fp64: clamp(conv3x3(silu(group_norm(x)), pad 1 of the ACTIVATED input) / 2 + 0.5, 0, 1) and the stats used."""
    x = x.double()
    N, C, H, W = x.shape
    xg = x.reshape(N, G, -1)
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + eps)
    a = ((xg - mean[..., None]) * rstd[..., None]).reshape(N, C, H, W) * gamma.double()[:, None, None] + beta.double()[:, None, None]
    a = F.silu(a)
    y = F.conv2d(a, w.double(), b.double(), padding=1)
    return (y / 2 + 0.5).clamp(0, 1)


def _call_head(x, mean, rstd, gamma, beta, w, b, G, prec=0, uint8=True):
    from mvip_nerf_amd._lib import call, ptr, stream
    N, C, H, W = x.shape
    img = torch.empty(N, 3, H, W, device=x.device)
    u8 = torch.empty(N, H, W, 3, device=x.device, dtype=torch.uint8) if uint8 else None
    call('mvip_vae_decoder_head', ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(w), ptr(b), N, C, H, W, G, 0, ptr(img),
         ptr(u8, torch.uint8), prec, stream())
    return img, u8


@pytest.mark.parametrize('shape', [(1, 128, 512, 512), (2, 64, 72, 104), (1, 32, 1, 1)])
def test_decoder_head_against_fp64(cuda, shape):
    from mvip_nerf_amd import ops
    N, C, H, W = shape
    G, eps = 32, 1e-6
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(shape, generator=g) * 1.7 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    w = torch.randn(3, C, 3, 3, generator=g) * (1.5 / math.sqrt(9 * C))
    b = torch.randn(3, generator=g) * 0.1
    ref = _head_ref64(x, gamma, beta, w, b, G, eps)
    xd = x.to(cuda)
    ws = ops._gn_workspace(N, C, H * W, cuda)
    mean, rstd = ops._gn_stats(xd, N, C, H, W, G, eps, ws)
    img, u8 = _call_head(xd, mean, rstd, gamma.to(cuda), beta.to(cuda), w.to(cuda), b.to(cuda), G)
    err = float((img.cpu().double() - ref).abs().max())
    print(f'head {shape}: max |img - fp64| = {err:.3e}')
    # images live in [0, 1]: absolute = relative to the range.  fp32 sums over 9 C taps: measured 2.5e-6 at 128 channels and
    # 512 x 512 (the largest of 786K outputs), 1.0e-6 at (2, 64, 72, 104), 5.4e-6 at 1 x 1 (one element per group: rstd =
    # 1/sqrt(eps) = 1000 amplifies the fp32 rounding of the mean); bound 2e-5 (3.7x headroom)
    assert err < 2e-5, err
    # uint8 = rint(255 img): equal except where the fp64 image value lies within 1e-4 of a .5 boundary (k + 0.5) / 255
    v = ref.permute(0, 2, 3, 1).numpy() * 255.0
    near = np.abs(v - np.floor(v) - 0.5) < 1e-4 * 255.0
    got = u8.cpu().numpy().astype(np.int32)
    want = np.rint(v).astype(np.int32)
    assert np.array_equal(got[~near], want[~near])
    assert np.all(np.abs(got[near] - want[near]) <= 1)
    assert (img.cpu() - img.cpu().clamp(0, 1)).abs().max() == 0


def test_decoder_head_pads_after_the_activation(cuda):
    """gamma = 0, beta = 2: the activation is silu(2) everywhere INSIDE the image; the border pixels' outputs sum only the
    in-image taps (padding of the activated input with 0), not silu(2) on the outside taps as well."""
    from mvip_nerf_amd import ops
    N, C, H, W, G = 1, 32, 5, 7, 32
    x = torch.randn(N, C, H, W, device=cuda)
    gamma, beta = torch.zeros(C, device=cuda), torch.full((C,), 2.0, device=cuda)
    w = torch.rand(3, C, 3, 3, device=cuda) * 0.02
    b = torch.full((3,), -1.0, device=cuda)
    mean, rstd = ops._gn_stats(x, N, C, H, W, G, 1e-6, ops._gn_workspace(N, C, H * W, cuda))
    img, _ = _call_head(x, mean, rstd, gamma, beta, w, b, G)
    s = 2.0 / (1.0 + math.exp(-2.0))
    wd = w.double().cpu().sum(1)                                # [3, 3, 3]: taps summed over the channels
    for (yy, xx) in [(0, 0), (0, 3), (H - 1, W - 1), (2, 0), (2, 3)]:
        taps = [(dy, dx) for dy in range(3) for dx in range(3) if 0 <= yy + dy - 1 < H and 0 <= xx + dx - 1 < W]
        for o in range(3):
            yv = -1.0 + s * sum(float(wd[o, dy, dx]) for dy, dx in taps)
            want = min(max(yv / 2 + 0.5, 0.0), 1.0)
            assert abs(float(img[0, o, yy, xx]) - want) < 2e-6, (yy, xx, o)
    # and the corner differs from what padding the PRE-activation input would give
    yv_wrong = -1.0 + s * float(wd[0].sum())
    assert abs(float(img[0, 0, 0, 0]) - (yv_wrong / 2 + 0.5)) > 1e-3


def test_decoder_head_argument_checks(cuda):
    from mvip_nerf_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 48, 4, 4, device=cuda)
    t = torch.zeros(64, device=cuda)
    img = torch.zeros(1, 3, 4, 4, device=cuda)
    P = lambda v: ctypes.c_void_p(v.data_ptr())
    null = ctypes.c_void_p(0)
    s = _lib.stream()
    args = lambda xp, C, imgp, dtype=0, prec=0: (xp, P(t), P(t), P(t), P(t), P(t), P(t), 1, C, 4, 4, 16, dtype, imgp, null, prec, s)
    assert lib.mvip_vae_decoder_head(*args(P(x), 48, P(img))) == -1            # C % 32 != 0
    assert lib.mvip_vae_decoder_head(*args(null, 32, P(img))) == -1            # null input
    assert lib.mvip_vae_decoder_head(*args(P(x), 32, null)) == -1              # null output
    assert lib.mvip_vae_decoder_head(*args(P(x), 32, P(img), dtype=2)) == -1
    assert lib.mvip_vae_decoder_head(*args(P(x), 32, P(img), prec=3)) == -1
    assert lib.mvip_ddim_cfg_step(null, 1, P(t), P(t), 16, null, 0, null, s) == -1
    assert lib.mvip_ddim_cfg_step(P(t), 1, P(t), P(t), 0, null, 0, null, s) == -1
    assert lib.mvip_ddim_cfg_step(P(t), 1, P(t), P(t), 16, P(t), 3, null, s) == -1  # UNet input with < 4 channels
    torch.cuda.synchronize()


@pytest.mark.parametrize('cfg', [True, False])
def test_ddim_step_kernel_against_fp64(cuda, cfg):
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_utils import ddim_step_scalars
    from mvip_nerf_amd.guidance.sd_nets import scaled_linear_alphas_cumprod
    alphas = [float(a) for a in scaled_linear_alphas_cumprod()]
    g = torch.Generator().manual_seed(1)
    B = 2 if cfg else 1
    eps = torch.randn(B, 4, 64, 64, generator=g)
    x = torch.randn(1, 4, 64, 64, generator=g)
    unet_in = torch.randn(B, 9, 64, 64, generator=g)
    sc = ddim_step_scalars(alphas, 981, 20, 7.5, t_next=961)
    scal = torch.zeros(6, device=cuda)
    for k, v in enumerate(sc):
        scal[k].fill_(v)
    s32 = scal.cpu().double()
    xd, ud, tout = x.to(cuda), unet_in.to(cuda), torch.zeros(1, device=cuda)
    ops.ddim_cfg_step(eps.to(cuda), xd, scal, ud, tout)
    e = eps.double()
    e = e[0:1] + s32[0] * (e[1:2] - e[0:1]) if cfg else e
    ref = s32[3] * (x.double() - s32[2] * e) / s32[1] + s32[4] * e
    err = float(((xd.cpu().double() - ref).abs() / ref.abs().max()).max())
    print(f'ddim cfg={cfg}: max error / max |x| = {err:.3e}')
    # measured 1.2e-6 (CFG, x0 amplified by 1/sqrt(abar_981) = 13.6) and 1.8e-7 of max |x|: a few ulps; bound 8e-6 (6.5x)
    assert err < 8e-6, err
    u = ud.cpu()
    for bb in range(B):
        assert torch.equal(u[bb, :4], xd.cpu()[0])               # the next UNet input's latent channels: the new latents, exactly
        assert torch.equal(u[bb, 4:], unet_in[bb, 4:])           # mask / masked-image channels untouched
    assert float(tout) == 961.0


def _rel_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm()), float(a @ b / (a.norm() * b.norm()))


def test_decode_latents_against_host_decoder(sd, cuda):
    """decode_latents on the device against the same AutoencoderKL evaluated on the host (torch ops): 512 x 512 in fp32,
    16 x 16 latents in fp64; then once in the --fp16 mode's single-product arithmetic."""
    vae_cpu = copy.deepcopy(sd.vae).cpu()
    g = torch.Generator().manual_seed(4)
    z = torch.randn(1, 4, 64, 64, generator=g)
    dev_img = sd.decode_latents(z.to(cuda)).cpu()
    with torch.no_grad():
        ref = (vae_cpu.decode(z / sd.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    rel, cos = _rel_cos(dev_img, ref)
    print(f'decode 512^2: rel L2 {rel:.3e} cos {cos:.8f}')
    assert dev_img.shape == (1, 3, 512, 512)
    assert rel < 1e-4 and cos > 0.99999, (rel, cos)             # measured 6.6e-7, cos 1 - 1e-9: fp32-grade (150x headroom)
    z16 = torch.randn(1, 4, 16, 16, generator=g)
    with torch.no_grad():
        ref16 = (copy.deepcopy(vae_cpu).double().decode(z16.double() / sd.scaling_factor)[0] / 2 + 0.5).clamp(0, 1)
    rel, cos = _rel_cos(sd.decode_latents(z16.to(cuda)).cpu(), ref16)
    print(f'decode 128^2 vs fp64: rel L2 {rel:.3e} cos {cos:.8f}')
    assert rel < 1e-4 and cos > 0.99999, (rel, cos)             # measured 3.6e-7
    prec = sd.vae.mfma_prec
    sd.vae.mfma_prec = 1                                        # the reference's --fp16 mode on the same kernels
    try:
        rel, cos = _rel_cos(sd.decode_latents(z.to(cuda)).cpu(), ref)
    finally:
        sd.vae.mfma_prec = prec
    print(f'decode 512^2 fp16 mode: rel L2 {rel:.3e} cos {cos:.8f}')
    assert rel < 2e-3 and cos > 0.9999, (rel, cos)              # measured 2.8e-4, cos 0.99999996 (one fp16 product; 7x)


def test_decode_latents_launches_no_library_kernel(sd, cuda):
    z = torch.randn(1, 4, 64, 64, device=cuda)
    sd.decode_latents(z)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        sd.decode_latents(z)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert not library_kernels_in(names), library_kernels_in(names)     # the banned names: tests/sd_network_cases.py
    for must in ('vae_decoder_head_kernel', 'conv3x3_f16x3_kernel'):
        assert any(must in n for n in names), must


def _explicit_loop(sd, emb, latents, cond, timesteps, ratio, gs):
    """Eager sd.unet calls + a torch fp64 DDIM update, written out."""
    a = sd._alphas_host
    x = latents.double()
    for t in timesteps:
        inp = torch.cat([torch.cat([x.float()] * 2), cond], 1)
        with torch.no_grad():
            eps = sd.unet(inp, t, encoder_hidden_states=emb, cross_attention_kwargs=None, return_dict=False)[0].double()
        e = eps[0:1] + gs * (eps[1:2] - eps[0:1])
        at, ap = a[t], (a[t - ratio] if t - ratio >= 0 else a[0])
        x = math.sqrt(ap) * (x - math.sqrt(1 - at) * e) / math.sqrt(at) + math.sqrt(1 - ap) * e
    return x


def test_produce_latents_replayed_equals_explicit_loop(sd, cuda):
    from mvip_nerf_amd.guidance.sd_utils import ddim_timesteps
    g = torch.Generator(device=cuda).manual_seed(9)
    lat = torch.randn(1, 4, 64, 64, device=cuda, generator=g)
    mask = (torch.rand(1, 1, 64, 64, device=cuda, generator=g) > 0.5).float()
    mlat = torch.randn(1, 4, 64, 64, device=cuda, generator=g)
    emb = sd.networks.encode_prompt(PROMPT, True)
    gs = 7.5
    ts, ratio = ddim_timesteps(4)
    replayed = sd.produce_latents(emb, num_inference_steps=4, guidance_scale=gs, latents=lat, mask=mask, masked_image_latents=mlat)
    assert sd.last_sample_steps == 4
    replayed2 = sd.produce_latents(emb, num_inference_steps=4, guidance_scale=gs, latents=lat, mask=mask, masked_image_latents=mlat)
    cond = torch.cat([torch.cat([mask] * 2), torch.cat([mlat] * 2)], 1)
    ref = _explicit_loop(sd, emb, lat, cond, ts, ratio, gs)
    sd.use_graphs = False
    try:
        eager = sd.produce_latents(emb, num_inference_steps=4, guidance_scale=gs, latents=lat, mask=mask, masked_image_latents=mlat)
    finally:
        sd.use_graphs = True
    r1 = float((replayed.double() - ref).norm() / ref.norm())
    r2 = float((eager.double() - ref).norm() / ref.norm())
    r3 = float((replayed - eager).norm() / eager.norm())
    print(f'sampler 4 steps: replayed vs explicit {r1:.3e}, eager vs explicit {r2:.3e}, replayed vs eager {r3:.3e}')
    # the bound of the graph-vs-eager SDS tests (test_sds.py): atomics level.  Measured 5.0e-7 against the explicit loop
    # (fp32 vs fp64 updates), replayed == eager bit for bit
    assert r1 < 1e-4 and r2 < 1e-4 and r3 < 1e-4, (r1, r2, r3)
    assert float((replayed - replayed2).norm() / replayed.norm()) < 1e-4


def test_inpaint_deterministic_api_and_strength(sd, cuda):
    g = torch.Generator(device=cuda).manual_seed(3)
    image = torch.rand(1, 3, 283, 504, device=cuda, generator=g)
    mask = torch.zeros(1, 1, 283, 504, device=cuda)
    mask[:, :, 70:210, 126:378] = 1
    runs = []
    for _ in range(2):
        sd.seed_generator(11)
        runs.append(sd.inpaint(image, mask, PROMPT, num_inference_steps=3))
    assert runs[0].shape == (1, 3, 512, 512)
    assert torch.equal(runs[0], runs[1])                     # same seed, same image
    assert float(runs[0].min()) >= 0 and float(runs[0].max()) <= 1
    sd.seed_generator(11)
    imgs = sd.prompt_to_img(PROMPT, num_inference_steps=2)
    assert isinstance(imgs, np.ndarray) and imgs.dtype == np.uint8 and imgs.shape == (1, 512, 512, 3)
    # strength 0.5 of 4 steps runs int(4 * 0.5) = 2 UNet forwards (counted on the eager path) and 2 replays on the graphed one
    sd.seed_generator(11)
    sd.inpaint(image, mask, PROMPT, num_inference_steps=4, strength=0.5)
    assert sd.last_sample_steps == 2
    calls = []
    fwd = sd.unet.forward
    sd.unet.forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
    sd.use_graphs = False
    try:
        sd.seed_generator(11)
        sd.inpaint(image, mask, PROMPT, num_inference_steps=4, strength=0.5)
    finally:
        sd.use_graphs = True
        del sd.unet.forward
    assert len(calls) == 2
    with pytest.raises(ValueError):
        sd.inpaint(image, mask, PROMPT, strength=0.0)
    with pytest.raises(NotImplementedError):
        sd.produce_latents(sd.networks.encode_prompt(PROMPT, True), height=256, width=256)
