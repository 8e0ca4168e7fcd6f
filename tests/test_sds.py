"""SDS wrapper arithmetic (train_step_sd / _sd_normal / _colla_sds, SpecifyGradient) on the GPU against
golden vectors produced by the reference's own wrapper running the same tiny stand-in networks
(oracle/gen_golden_sds.py).  Random draws are replayed from the recorded CPU seed."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sd_network_cases import large_mean_residual                       # noqa: E402

from oracle.sds_standin import TinyVAE, TinyUNet, TinyScheduler, prompt_embedding   # noqa: E402

pytestmark = pytest.mark.gpu


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def make_sd(dev, seed, n_draws):
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    cache = {}

    def encode_prompt(p, cfg):               # cached on the device (a graph capture cannot contain H2D copies)
        if (p, cfg) not in cache:
            cache[(p, cfg)] = prompt_embedding(p, cfg).to(dev)
        return cache[(p, cfg)]
    nets = types.SimpleNamespace(vae=TinyVAE().to(dev), unet=TinyUNet().to(dev), encode_prompt=encode_prompt,
                                 alphas_cumprod=TinyScheduler().alphas_cumprod)
    sd = StableDiffusion(dev, False, False, networks=nets)
    torch.manual_seed(int(seed))
    draws = [torch.randn(1, 4, 64, 64) for _ in range(n_draws)]          # the reference's CPU draws, in order
    it = iter(draws)
    sd._randn = lambda shape, dtype=torch.float32: next(it).to(dev)
    return sd


@pytest.mark.parametrize('i', [0, 100, 5000, 20000])
def test_train_step_sd_golden(golden, cuda, i):
    g = golden(f'sds_rgb_i{i}')
    sd = make_sd(cuda, g['seed'], 4)
    pred = T(g['pred'], cuda).requires_grad_(True)
    loss = sd.train_step_sd(int(g['i']), T(g['mask'], cuda), 'a stone bench in a park', pred,
                            guidance_scale=float(g['guidance_scale']), as_latent=True, grad_scale=1)
    assert loss.shape == (1,) and float(loss) == 1.0
    (float(g['upstream']) * loss).sum().backward()
    scale = np.abs(g['d_pred']).max()
    np.testing.assert_allclose(N(pred.grad), g['d_pred'], rtol=2e-3, atol=2e-4 * scale)


def test_sds_internals_golden(golden, cuda):
    """latents, the SDS gradient and the 64x64 mask handed to SpecifyGradient."""
    from mvip_nerf_amd.guidance import sd_utils
    g = golden('sds_rgb_i5000')
    sd = make_sd(cuda, g['seed'], 4)
    seen = {}
    orig = sd_utils.SpecifyGradient.apply

    def spy(latents, grad, mask):
        seen.update(latents=latents.detach(), grad=grad.detach(), mask=mask.detach())
        return orig(latents, grad, mask)
    sd_utils.SpecifyGradient.apply = staticmethod(spy)
    try:
        sd.train_step_sd(int(g['i']), T(g['mask'], cuda), 'a stone bench in a park', T(g['pred'], cuda),
                         guidance_scale=float(g['guidance_scale']))
    finally:
        sd_utils.SpecifyGradient.apply = orig
    assert sd._timestep(np.sqrt(5000 / 20000)) == 500
    np.testing.assert_array_equal(N(seen['mask']), g['mask64'])
    np.testing.assert_allclose(N(seen['latents']), g['latents'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(seen['grad']), g['grad'], rtol=1e-3, atol=1e-4 * np.abs(g['grad']).max())


def test_train_step_sd_normal_golden(golden, cuda):
    g = golden('sds_normal')
    sd = make_sd(cuda, g['seed'], 4)
    pred = T(g['pred'], cuda).requires_grad_(True)
    loss = sd.train_step_sd_normal(int(g['i']), T(g['mask'], cuda), 'a normal map of a stone bench', pred,
                                   guidance_scale=float(g['guidance_scale']), normal_start=int(g['normal_start']))
    (float(g['upstream']) * loss).sum().backward()
    scale = np.abs(g['d_pred']).max()
    np.testing.assert_allclose(N(pred.grad), g['d_pred'], rtol=2e-3, atol=2e-4 * scale)


def test_train_step_colla_golden(golden, cuda):
    """Reproduces the reference's behaviour as written: only the last view gets gradient, x2 from the
    CFG-duplicated mask, accumulated grad."""
    g = golden('sds_colla')
    sd = make_sd(cuda, g['seed'], 12)
    preds = T(g['preds'], cuda).requires_grad_(True)
    loss = sd.train_step_colla_sds(1234, T(g['masks'], cuda), 'a stone bench in a park', preds,
                                   guidance_scale=float(g['guidance_scale']))
    (float(g['upstream']) * loss).sum().backward()
    d = N(preds.grad)
    assert np.abs(d[:-1]).max() == 0.0 and np.abs(g['d_preds'][:-1]).max() == 0.0
    scale = np.abs(g['d_preds']).max()
    np.testing.assert_allclose(d, g['d_preds'], rtol=2e-3, atol=2e-4 * scale)


def test_sds_elementwise_kernels(cuda):
    from mvip_nerf_amd.guidance.sd_utils import sds_grad, _AddNoise
    gen = torch.Generator(device=cuda).manual_seed(0)
    eu, ec, nz = (torch.randn(1, 4, 64, 64, device=cuda, generator=gen) for _ in range(3))
    eu[0, 0, 0, 0] = float('nan'); ec[0, 0, 0, 1] = float('inf'); nz[0, 0, 0, 2] = float('inf')
    got = sds_grad(eu, ec, nz, 7.5, 0.37)
    ref = torch.nan_to_num(0.37 * (eu + 7.5 * (ec - eu) - nz))
    np.testing.assert_allclose(N(got), N(ref), rtol=1e-6, atol=1e-6)
    x0 = torch.randn(1, 4, 64, 64, device=cuda, generator=gen).requires_grad_(True)
    out = _AddNoise.apply(x0, nz.nan_to_num(), 0.8, 0.6)
    np.testing.assert_allclose(N(out), N(0.8 * x0 + 0.6 * nz.nan_to_num()), rtol=1e-6, atol=1e-6)
    out.sum().backward()
    np.testing.assert_allclose(N(x0.grad), 0.8, rtol=1e-6)


@pytest.mark.parametrize('shape,size', [((1, 3, 378, 504), (512, 512)), ((1, 4, 567, 1008), (512, 512)),
                                        ((2, 1, 20, 28), (512, 512)), ((1, 3, 600, 512), (512, 512)),
                                        ((1, 2, 7, 5), (3, 11)), ((1, 1, 1, 9), (4, 4))])
def test_resize_bilinear_vs_torch(cuda, shape, size):
    """ops.resize_bilinear (the resize in front of vae.encode) and its gather-form adjoint vs F.interpolate and its
    autograd on the same device tensors; fp32 with the same source-index arithmetic, so agreement is to rounding."""
    from mvip_nerf_amd import ops
    g = torch.Generator().manual_seed(sum(shape) + size[1])
    x = torch.randn(shape, generator=g).to(cuda)
    dy = torch.randn(shape[:2] + size, generator=g).to(cuda)
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.interpolate(xr, size, mode='bilinear', align_corners=False)
    ref.backward(dy)
    xh = x.clone().requires_grad_(True)
    got = ops.resize_bilinear(xh, size)
    got.backward(dy)
    np.testing.assert_allclose(N(got), N(ref), rtol=0, atol=2e-6)
    np.testing.assert_allclose(N(xh.grad), N(xr.grad), rtol=0, atol=2e-5 * max(1.0, float(xr.grad.abs().max())))
    # adjoint identity <J x, dy> = <x, J^T dy> in fp64
    lhs = float((got.detach().double() * dy.double()).sum())
    rhs = float((x.double() * xh.grad.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs))


@pytest.mark.parametrize('N_,cin,cout,H,W,k,stride,pad,pads', [
    (2, 320, 320, 64, 64, 3, 2, 1, None),            # UNet down-sampler
    (1, 128, 128, 64, 96, 3, 2, 0, (0, 0, 1, 1)),    # VAE down-sampler: bottom / right padding only
    (1, 3, 128, 64, 64, 3, 1, 1, None),              # VAE conv_in (K = 27 -> 32)
    (2, 9, 320, 32, 32, 3, 1, 1, None),              # UNet conv_in (K = 81 -> 96)
    (2, 320, 4, 32, 32, 3, 1, 1, None),              # UNet conv_out (M = 4 -> 32)
    (1, 8, 8, 16, 16, 1, 1, 0, None),                # quant_conv
    (2, 160, 96, 16, 16, 3, 2, 1, None),             # 8 x 8 output: P = 64 -> 256
    (1, 5, 7, 13, 11, 3, 2, 1, None)])               # odd everything
def test_conv_gemm_vs_fp64(cuda, N_, cin, cout, H, W, k, stride, pad, pads):
    """ops.conv_gemm (im2col split planes + the split-precision GEMM; data gradient = transposed GEMM + col2im gather)
    vs F.conv2d in fp64 on the host, forward and input gradient."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import conv_any
    gen = torch.Generator().manual_seed(cin * 7 + cout + H)
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=pad)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (k * k * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    for p in conv.parameters():
        p.requires_grad_(False)
    x = torch.randn(N_, cin, H, W, generator=gen) * 0.7 + 0.1
    xr = x.double().requires_grad_(True)
    xp = xr if pads is None else torch.nn.functional.pad(xr, (pads[1], pads[3], pads[0], pads[2]))
    yr = torch.nn.functional.conv2d(xp, conv.weight.double(), conv.bias.double(), stride=stride, padding=pad)
    dy = torch.randn(yr.shape, generator=gen) * 1e-4
    yr.backward(dy.double())
    conv_d = conv.to(cuda)
    xd = x.to(cuda).requires_grad_(True)
    assert ops.conv_gemm_supported(conv_d, xd)
    y = conv_any(conv_d, xd, pads)
    assert y.shape == yr.shape
    np.testing.assert_allclose(N(y), yr.detach().float().numpy(), rtol=0, atol=1e-5 * float(yr.abs().max()))
    y.backward(dy.to(cuda))
    np.testing.assert_allclose(N(xd.grad), xr.grad.float().numpy(), rtol=0, atol=1e-5 * float(xr.grad.abs().max()))


def test_pretrain_model_dispatch(cuda):
    """cal_loss sums the enabled terms in the reference's order and gates colla on i>0, normal on i>normal_start."""
    from mvip_nerf_amd.nerf.utils import Pretrain_Model

    class FakeSD(torch.nn.Module):
        calls = []

        def train_step_sd(self, i, *a, **k):
            self.calls.append('rgb'); return torch.tensor([1.0])

        def train_step_colla_sds(self, i, *a, **k):
            self.calls.append('colla'); return torch.tensor([10.0])

        def train_step_sd_normal(self, i, *a, **k):
            self.calls.append('normal'); return torch.tensor([100.0])

    opt = types.SimpleNamespace(is_rgb_guidance=True, is_colla_guidance=True, is_normal_guidance=True, text='t',
                                text_normal='n', rgb_guidance_scale=7.5, colla_guidance_scale=7.5,
                                normal_guidance_scale=1.5, normal_start=500, lambda_guidance=1)
    pm = Pretrain_Model(opt, cuda, {'SD': FakeSD()})
    assert float(pm.cal_loss(0, None, None, None, None, None, None, None)) == 1.0
    assert float(pm.cal_loss(10, None, None, None, None, None, None, None)) == 11.0
    assert float(pm.cal_loss(501, None, None, None, None, None, None, None)) == 111.0
    assert FakeSD.calls == ['rgb', 'rgb', 'colla', 'rgb', 'colla', 'normal'] and pm.global_step == 3


def test_graphed_step_equals_eager(golden, cuda):
    """use_graphs=True replays a captured hipGraph of the whole step (incl. the VAE-encoder backward);
    with the same noise it must give the eager gradient, for several timesteps through ONE graph."""
    import itertools
    g = golden('sds_rgb_i100')
    torch.manual_seed(3)
    fixed = [torch.randn(1, 4, 64, 64, device=cuda) for _ in range(4)]
    outs = {}
    for mode in (False, True):
        sd = make_sd(cuda, 0, 0)
        sd.use_graphs = mode
        cyc = itertools.cycle(fixed)
        sd._randn = lambda shape, dtype=torch.float32: next(cyc)
        res = []
        for i in (100, 5000, 19000):
            pred = T(g['pred'], cuda).requires_grad_(True)
            loss = sd.train_step_sd(i, T(g['mask'], cuda), 'a stone bench in a park', pred, guidance_scale=7.5)
            (1e-4 * loss).sum().backward()
            res.append(N(pred.grad))
        outs[mode] = res
        if mode:
            assert len(sd._graphs) == 1
    for a, b in zip(outs[False], outs[True]):
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-6 * np.abs(a).max())
    assert not np.allclose(outs[True][0], outs[True][2])       # the timestep really changed between replays


# GroupNorm (+SiLU) of the SDS networks: HIP kernel pair vs the fp64 statement of the same op on the host.
# Tolerance: fp32 5e-6 relative to the output scale (statistics are fp64 in the kernel); fp16 storage 2e-3.
@pytest.mark.parametrize('shape,groups', [((2, 320, 64, 64), 32), ((1, 128, 96, 96), 32), ((2, 64, 7, 9), 32),
                                           ((1, 64, 3, 5), 32), ((1, 128, 512, 512), 32), ((2, 2560, 8, 8), 32),
                                           ((3, 12, 5), 4)])
@pytest.mark.parametrize('silu', [False, True])
def test_group_norm_forward_backward(cuda, shape, groups, silu):
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(sum(shape) + int(silu))
    C = shape[1]
    x = (torch.randn(shape, generator=gen) * 1.7 + 0.9)
    w = torch.randn(C, generator=gen) * 0.5 + 1.0
    b = torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(shape, generator=gen)
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.group_norm(xr, groups, w.double(), b.double(), 1e-6)
    if silu:
        yr = torch.nn.functional.silu(yr)
    yr.backward(dy.double())
    xd = x.to(cuda).requires_grad_(True)
    y = ops.group_norm(xd, w.to(cuda), b.to(cuda), groups, 1e-6, silu)
    y.backward(dy.to(cuda))
    ys, gs = float(yr.abs().max()), float(xr.grad.abs().max())
    np.testing.assert_allclose(N(y), yr.detach().float().numpy(), rtol=0, atol=5e-6 * max(ys, 1.0))
    np.testing.assert_allclose(N(xd.grad), xr.grad.float().numpy(), rtol=0, atol=5e-6 * max(gs, 1e-3))


def test_group_norm_fp16_and_errors(cuda):
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 32, 32, generator=gen)
    w, b = torch.randn(64, generator=gen), torch.randn(64, generator=gen)
    ref = torch.nn.functional.silu(torch.nn.functional.group_norm(x.half().double(), 32, w.half().double(),
                                                                  b.half().double(), 1e-5))
    xh = x.half().to(cuda).requires_grad_(True)
    y = ops.group_norm(xh, w.half().to(cuda), b.half().to(cuda), 32, 1e-5, True)
    assert y.dtype == torch.float16
    np.testing.assert_allclose(N(y.float()), ref.float().numpy(), rtol=2e-3, atol=2e-3)
    y.float().sum().backward()
    assert xh.grad.dtype == torch.float16 and torch.isfinite(xh.grad).all()
    # same values as the modules of sd_nets produce through torch on the host
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm
    m = GroupNorm(32, 64, eps=1e-5)
    with torch.no_grad():
        m.weight.copy_(w); m.bias.copy_(b)
    m.requires_grad_(False)
    host = m(x, silu=True)
    dev = m.to(cuda)(x.to(cuda), silu=True)
    np.testing.assert_allclose(N(dev), host.detach().numpy(), rtol=0, atol=2e-5)
    with pytest.raises(NotImplementedError):
        ops.group_norm(x.to(cuda), w.to(cuda).requires_grad_(True), b.to(cuda), 32, 1e-5, False)
    with pytest.raises(Exception):
        ops.group_norm(x.to(cuda), w.to(cuda), b.to(cuda), 7, 1e-5, False)       # C % G != 0


# GroupNorm + SiLU + 3x3 convolution (+ channel addend + residual) on the split-precision MFMA kernel vs the
# same expression in fp64 on the host.  Tolerance 1e-5 of the output / gradient scale (fp16 hi+lo operands,
# three products, fp32 accumulation: ~1e-6 relative).
@pytest.mark.parametrize('N_,cin,cout,H,W,grad', [(1, 32, 64, 8, 32, False), (2, 128, 128, 16, 64, True),
                                                  (1, 64, 128, 24, 96, True), (1, 128, 256, 8, 32, True),
                                                  (1, 16, 64, 8, 32, False), (1, 160, 64, 8, 64, True),
                                                  (2, 320, 320, 32, 32, True), (2, 64, 64, 16, 16, True),
                                                  (1, 128, 64, 32, 16, True), (2, 160, 96, 16, 48, False),    # these three: 16x16 tiles
                                                  (1, 128, 128, 256, 256, True), (1, 64, 96, 256, 256, False),    # large frames (eight-wave tiles when MVIP_CONV_WIDE=1)
                                                  (2, 320, 64, 8, 8, True), (5, 160, 96, 8, 8, True),             # 8x8 images (four per workgroup), channel splits
                                                  (2, 640, 64, 16, 16, True), (1, 256, 32, 8, 32, False)])        # channel splits on the 16x16 and 8x32 tiles
def test_norm_act_conv3x3(cuda, N_, cin, cout, H, W, grad):
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm, norm_act_conv
    gen = torch.Generator().manual_seed(cin + cout + H)
    G = 8 if cin < 32 else 32
    norm = GroupNorm(G, cin, eps=1e-6)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(cin, generator=gen) * 0.4 + 1.0)
        norm.bias.copy_(torch.randn(cin, generator=gen) * 0.3)
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (9 * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    for p in list(norm.parameters()) + list(conv.parameters()):
        p.requires_grad_(False)
    x = torch.randn(N_, cin, H, W, generator=gen) * 1.3 + 0.2
    ca = torch.randn(N_, cout, generator=gen)
    rs = torch.randn(N_, cout, H, W, generator=gen)
    dy = torch.randn(N_, cout, H, W, generator=gen) * 1e-5          # gradients are tiny in the SDS step
    # fp64 statement on the host
    xr, car, rsr = (t.double().requires_grad_(grad) for t in (x, ca, rs))
    h = torch.nn.functional.silu(torch.nn.functional.group_norm(xr, G, norm.weight.double(), norm.bias.double(), 1e-6))
    yr = torch.nn.functional.conv2d(h, conv.weight.double(), conv.bias.double(), padding=1) + car[:, :, None, None] + rsr
    # device
    norm_d, conv_d = norm.to(cuda), conv.to(cuda)
    xd, cad, rsd = (t.to(cuda).requires_grad_(grad) for t in (x, ca, rs))
    assert ops.conv3x3_supported(conv_d, xd)
    y = norm_act_conv(norm_d, conv_d, xd, chan_add=cad, residual=rsd)
    ys = float(yr.abs().max())
    np.testing.assert_allclose(N(y), yr.detach().float().numpy(), rtol=0, atol=1e-5 * ys)
    if grad:
        yr.backward(dy.double())
        y.backward(dy.to(cuda))
        for got, ref in ((xd.grad, xr.grad), (cad.grad, car.grad), (rsd.grad, rsr.grad)):
            np.testing.assert_allclose(N(got), ref.float().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))


def test_resnet_block_fused_equals_library_path(cuda):
    """The SD ResNet block through the fused HIP path equals the same block through GroupNorm kernels + the
    library convolution (shape the MFMA kernel does not cover is forced by making the width 48)."""
    from mvip_nerf_amd.guidance.sd_nets import ResnetBlock2D
    torch.manual_seed(3)
    blk = ResnetBlock2D(128, 256, temb=64).to(cuda)
    for p in blk.parameters():
        p.requires_grad_(False)
    x = torch.randn(1, 128, 16, 64, device=cuda)
    temb = torch.randn(1, 64, device=cuda)
    fused = blk(x, temb)
    x48 = torch.nn.functional.pad(x, (0, 0, 0, 0))          # same data; library path via the CPU module
    ref = blk.to('cpu').double()(x48.cpu().double(), temb.cpu().double())
    np.testing.assert_allclose(N(fused), ref.float().numpy(), rtol=0, atol=2e-5 * float(ref.abs().max()))


def test_identity_shortcut_chain_gradient(cuda):
    """Three VAE-style ResNet blocks in a row (identity shortcuts) under autograd: the shortcut gradient is added inside the
    first convolution's GroupNorm backward (ops.ShortcutLink) and every block's dy takes its power-of-two scale from the
    per-workgroup maxima its producer left (mvip_groupnorm_backward_fused / mvip_absmax_scale_from_maxima).  Checked
    against the same chain in fp64 on the host, and bit for bit against the unlinked path with the absmax passes (the
    scales are the same powers of two; only the order of one fp32 addition differs... none does: a + b is commutative)."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import ResnetBlock2D
    torch.manual_seed(11)
    blks = [ResnetBlock2D(128, 128, eps=1e-6) for _ in range(3)]
    for b in blks:
        for p in b.parameters():
            p.requires_grad_(False)
    x = torch.randn(1, 128, 40, 64) * 1.5 + 0.3
    dy = torch.randn(1, 128, 40, 64) * 1e-5
    xr = x.double().requires_grad_(True)
    h = xr
    for b in blks:
        h = b.double()(h)
    h.backward(dy.double())
    blks = [b.float().to(cuda) for b in blks]

    def run(linked):
        xd = x.to(cuda).requires_grad_(True)
        old = ops.ShortcutLink
        calls = []
        orig_call = ops.call

        def counting(name, *a):
            calls.append(name)
            return orig_call(name, *a)
        ops.call = counting
        try:
            if not linked:
                class _NoLink:                      # never picked up: norm_act_conv gets link=None
                    def __new__(cls):
                        return None
                ops.ShortcutLink = _NoLink
            hd = xd
            for b in blks:
                hd = b(hd)
            if not linked:
                ops._LAST_DX[0] = None
            hd.backward(dy.to(cuda))
        finally:
            ops.ShortcutLink, ops.call = old, orig_call
        return hd.detach(), xd.grad, calls
    y1, g1, calls1 = run(True)
    assert calls1.count('mvip_absmax_scale_from_maxima') == 5 and calls1.count('mvip_absmax_scale') == 1, calls1
    np.testing.assert_allclose(N(y1), h.detach().float().numpy(), rtol=0, atol=2e-5 * float(h.abs().max()))
    np.testing.assert_allclose(N(g1), xr.grad.float().numpy(), rtol=0, atol=2e-5 * float(xr.grad.abs().max()))
    # the unlinked path: autograd adds the shortcut gradient, every dy is re-read for its maximum
    orig = ops._scale_of_gradient

    def always_absmax(dyc):
        ops._LAST_DX[0] = None
        return orig(dyc)
    ops._scale_of_gradient = always_absmax
    try:
        y0, g0, calls0 = run(False)
    finally:
        ops._scale_of_gradient = orig
    assert calls0.count('mvip_absmax_scale_from_maxima') == 0 and calls0.count('mvip_absmax_scale') == 6
    assert torch.equal(y0, y1) and torch.equal(g0, g1)


@pytest.mark.parametrize('N_,cin,cout,H,W', [(2, 320, 320, 64, 64), (2, 640, 640, 32, 32), (2, 320, 640, 16, 16), (2, 1280, 1280, 8, 8)])
def test_split_reduction_leaves_row_moments(cuda, N_, cin, cout, H, W):
    """A channel-split convolution's reduction launch also writes the GroupNorm row moments of its output
    (mvip_conv3x3_f16x3_ws_moments): y bit-identical to the plain launch, moments equal to mvip_groupnorm_stats' partials
    (fp64, a different summation order: 1e-12), and the next forward-only GroupNorm uses them (no gn_moments pass)."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd.ops import call, ptr, stream
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm, norm_act_conv
    lib = _lib.load()
    assert int(lib.mvip_conv3x3_row_moments_doubles(N_, cin, cout, H, W)) == N_ * cout * 2
    g = torch.Generator(device=cuda).manual_seed(cin + H)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(cuda)
    x = torch.randn(N_, cin, H, W, device=cuda, generator=g)
    rs = torch.randn(N_, cout, H, W, device=cuda, generator=g) * 2 + 1.5
    ca = torch.randn(N_, cout, device=cuda, generator=g)
    s2 = ops.absmax_scale(x)
    xs = ops._split_buffer(N_, cin, H * W, cuda)
    call('mvip_split_planes', ptr(x), N_, cin, H * W, ptr(s2), ptr(xs, torch.float16), 0, stream())
    packed, bias = ops._conv_packed(conv, False), conv.bias.detach().contiguous()
    y0, y1 = torch.empty(N_, cout, H, W, device=cuda), torch.empty(N_, cout, H, W, device=cuda)
    ops._conv3x3_launch(xs, packed, bias, ca, rs, s2, N_, cin, cout, H, W, y0)
    ops._LAST_Y[0] = None
    ops._conv3x3_launch(xs, packed, bias, ca, rs, s2, N_, cin, cout, H, W, y1, moments=True)
    assert torch.equal(y0, y1)
    assert ops._LAST_Y[0] is not None and ops._LAST_Y[0][0] is y1
    rm = ops._LAST_Y[0][2]
    ws = ops._gn_workspace(N_, cout, H * W, cuda)
    assert ws.numel() == rm.numel()
    call('mvip_groupnorm_stats', ptr(y1), N_, cout, H * W, 32, 1e-5, 0, None, None, ptr(ws, torch.float64), stream())
    np.testing.assert_allclose(rm.cpu().numpy(), ws.cpu().numpy(), rtol=1e-11, atol=1e-9)
    # the consumer: a forward-only norm -> silu -> conv takes the registered moments (and no gn_moments pass runs)
    norm = GroupNorm(32, cout).to(cuda)
    conv2 = torch.nn.Conv2d(cout, 64, 3, padding=1).to(cuda)
    for p in list(norm.parameters()) + list(conv2.parameters()):
        p.requires_grad_(False)
    calls = []
    orig = ops.call

    def counting(name, *a):
        calls.append(name)
        return orig(name, *a)
    ops.call = counting
    try:
        with torch.no_grad():
            z1 = norm_act_conv(norm, conv2, y1)
            z0 = norm_act_conv(norm, conv2, y0)            # nothing registered for y0: the ordinary path
    finally:
        ops.call = orig
    assert calls.count('mvip_groupnorm_stats') == 1 and calls.count('mvip_groupnorm_split_planes_moments') == 2
    np.testing.assert_allclose(N(z1), N(z0), rtol=0, atol=1e-6 * float(z0.abs().max()))
    y1.add_(1.0)                                           # modified in place: registered moments no longer describe it
    ops._LAST_Y[0] = (y1, 0, rm)
    assert ops._row_moments_of(y1) is None


@pytest.mark.parametrize('N_,cin,cout,H,W', [(1, 128, 128, 256, 256), (2, 320, 320, 64, 64), (1, 128, 256, 128, 128), (1, 64, 128, 128, 256),
                                             (3, 128, 128, 128, 128)])
def test_unsplit_convolution_leaves_moments_from_its_epilogue(cuda, N_, cin, cout, H, W):
    """Round 6 (VERDICT r5 task 2): an UNSPLIT convolution leaves the GroupNorm moments of its output too
    (mvip_conv3x3_f16x3_tile_moments: fp32 partials per pixel tile and wave from the epilogue -- five DPP adds per channel --
    summed in fp64 by a small second launch): y bit-identical to the plain launch, the moments equal to mvip_groupnorm_stats'
    partial sums of y at the accuracy of a 64-term fp32 sum (<= 4e-6 of sum |y| resp. sum y^2, mean offset included: the
    residual carries one), and the next forward-only GroupNorm consumes them without a pass over y.  A channel-split shape keeps
    its own route (scratch bytes = 0)."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd.ops import call, ptr, stream
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm, norm_act_conv
    lib = _lib.load()
    sb = int(lib.mvip_conv3x3_tile_moments_scratch_bytes(N_, cin, cout, H, W))
    split = int(lib.mvip_conv3x3_workspace_bytes(N_, cin, cout, H, W)) > 0
    assert (sb == 0) == split
    if split:
        assert (N_, H) == (2, 64)                          # the UNet's 64 x 64 level at 320 channels: 160 workgroups, channel-split
        return
    g = torch.Generator(device=cuda).manual_seed(cin + H)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(cuda)
    x = torch.randn(N_, cin, H, W, device=cuda, generator=g)
    rs = torch.randn(N_, cout, H, W, device=cuda, generator=g) * 2 + 1.5
    ca = torch.randn(N_, cout, device=cuda, generator=g)
    s2 = ops.absmax_scale(x)
    xs = ops._split_buffer(N_, cin, H * W, cuda)
    call('mvip_split_planes', ptr(x), N_, cin, H * W, ptr(s2), ptr(xs, torch.float16), 0, stream())
    packed, bias = ops._conv_packed(conv, False), conv.bias.detach().contiguous()
    y0, y1 = torch.empty(N_, cout, H, W, device=cuda), torch.empty(N_, cout, H, W, device=cuda)
    ops._conv3x3_launch(xs, packed, bias, ca, rs, s2, N_, cin, cout, H, W, y0)
    ops._LAST_Y[0] = None
    ops._conv3x3_launch(xs, packed, bias, ca, rs, s2, N_, cin, cout, H, W, y1, moments=True)
    assert torch.equal(y0, y1)
    assert ops._LAST_Y[0] is not None and ops._LAST_Y[0][0] is y1
    rm = ops._LAST_Y[0][2]
    ws = ops._gn_workspace(N_, cout, H * W, cuda)
    assert ws.numel() == rm.numel()
    chunks = rm.numel() // (N_ * cout * 2)
    got = rm.reshape(N_ * cout, chunks, 2).sum(1).cpu().numpy()
    yd = y1.double().reshape(N_ * cout, -1)
    want = torch.stack([yd.sum(1), (yd * yd).sum(1)], 1).cpu().numpy()
    scale = torch.stack([yd.abs().sum(1), (yd * yd).sum(1)], 1).cpu().numpy()
    assert np.abs(got - want).max() <= 4e-6 * scale.max() and (np.abs(got - want) <= 4e-6 * scale).all()
    assert float(rm.reshape(N_ * cout, chunks, 2)[:, 1:].abs().max()) == 0.0 if chunks > 1 else True
    norm = GroupNorm(32, cout).to(cuda)
    conv2 = torch.nn.Conv2d(cout, 64, 3, padding=1).to(cuda)
    for p in list(norm.parameters()) + list(conv2.parameters()):
        p.requires_grad_(False)
    calls = []
    orig = ops.call

    def counting(name, *a):
        calls.append(name)
        return orig(name, *a)
    ops.call = counting
    try:
        with torch.no_grad():
            z1 = norm_act_conv(norm, conv2, y1)
            z0 = norm_act_conv(norm, conv2, y0)            # nothing registered for y0: the ordinary path
    finally:
        ops.call = orig
    assert calls.count('mvip_groupnorm_stats') == 1 and calls.count('mvip_groupnorm_split_planes_moments') == 2
    np.testing.assert_allclose(N(z1), N(z0), rtol=0, atol=2e-6 * float(z0.abs().max()))


@pytest.mark.parametrize('per_channel', [False, True])
@pytest.mark.parametrize('ratio', [10, 30, 100])
@pytest.mark.parametrize('N_,cin,cout,H,W', [(1, 16, 128, 8, 32), (1, 16, 128, 16, 16), (2, 64, 256, 32, 64)])
def test_epilogue_moments_under_a_large_group_mean(cuda, N_, cin, cout, H, W, ratio, per_channel):
    """The moments an unsplit convolution leaves from its epilogue, judged by what their consumer makes of them when the
    output's group mean is 10, 30 and 100 standard deviations (residual streams; a variance formed as E[y^2] - mean^2 from
    fp32 squares loses (mean / std)^2 ulps): norm_act_conv(norm, conv2, y) with the registered moments against GroupNorm ->
    SiLU -> convolution of the same y in fp64 on the host.  The measure is the same consumer with the registration cleared
    (mvip_groupnorm_stats: a pass over y in fp64) against the same reference: the registered route may err 4x as much, with
    a floor of 3e-6 of the output scale (the grade of the split-precision convolution itself).
    Shapes: the smallest for which mvip_conv3x3_tile_moments_scratch_bytes(...) > 0 AND whose moments the next GroupNorm
    takes (four channels per group: Cout = 128) -- one 8 x 32 tile (Cin = 16: fewer than four channel chunks are never
    split), one 16 x 16 tile -- and a larger one of two images, eight tiles each and eight channels per group.
    Measured on an MI355X, registered / two-pass error of max |z|.  With the epilogue summing raw fp32 squares (as it did when
    this test was written) 10 of the 18 cases missed the bound: 7.5e-6 / 6.5e-7 and 8.2e-6 / 5.2e-7 at mean / std 28,
    1.08e-4 / 2.0e-6 at 93 and 7.2e-5 / 1.7e-6 at 70 (16 x 16 tile); 2.7e-5 / 2.0e-6 at 93 (two images).  With the squares taken
    about a shift, one of the wave's own 64 values (what the epilogue does now): 4.1e-7 / 3.8e-7 at 9, 7.1e-7 / 6.8e-7 at 28,
    2.28e-6 / 2.26e-6 at 93, 1.58e-6 / 1.60e-6 at 69 -- the two routes agree to 10 % in every case."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd.ops import call, ptr, stream
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm, norm_act_conv
    lib = _lib.load()
    assert int(lib.mvip_conv3x3_tile_moments_scratch_bytes(N_, cin, cout, H, W)) > 0
    assert int(lib.mvip_conv3x3_workspace_bytes(N_, cin, cout, H, W)) == 0
    gen = torch.Generator().manual_seed(cout + H + ratio)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    norm = GroupNorm(32, cout)
    conv2 = torch.nn.Conv2d(cout, 64, 3, padding=1)
    with torch.no_grad():
        norm.weight.add_(torch.randn(cout, generator=gen) * 0.2)
        norm.bias.add_(torch.randn(cout, generator=gen) * 0.2)
    for p in list(conv.parameters()) + list(norm.parameters()) + list(conv2.parameters()):
        p.requires_grad_(False)
    x = torch.randn(N_, cin, H, W, generator=gen) * 0.3              # conv(x): standard deviation ~0.17, the residual's is 0.5
    rs = large_mean_residual((N_, cout, H, W), ratio, per_channel, gen)
    ca = torch.randn(N_, cout, generator=gen) * 0.1
    host = [t.detach().double().clone() for t in (norm.weight, norm.bias, conv2.weight, conv2.bias)]     # .to(cuda) moves the modules
    conv_d, norm_d, conv2_d = conv.to(cuda), norm.to(cuda), conv2.to(cuda)
    xd, rsd, cad = x.to(cuda), rs.to(cuda), ca.to(cuda)
    s2 = ops.absmax_scale(xd)
    xs = ops._split_buffer(N_, cin, H * W, cuda)
    call('mvip_split_planes', ptr(xd), N_, cin, H * W, ptr(s2), ptr(xs, torch.float16), 0, stream())
    packed, bias = ops._conv_packed(conv_d, False), conv_d.bias.detach().contiguous()
    y0, y1 = torch.empty(N_, cout, H, W, device=cuda), torch.empty(N_, cout, H, W, device=cuda)
    ops._conv3x3_launch(xs, packed, bias, cad, rsd, s2, N_, cin, cout, H, W, y0)
    ops._LAST_Y[0] = None
    ops._conv3x3_launch(xs, packed, bias, cad, rsd, s2, N_, cin, cout, H, W, y1, moments=True)
    assert torch.equal(y0, y1)                                       # the moments cost y no bit
    assert ops._LAST_Y[0] is not None and ops._LAST_Y[0][0] is y1
    y64 = y1.cpu().double()
    yg = y64.reshape(N_, 32, -1)
    got_ratio = float((yg.mean(-1).abs() / yg.std(-1)).median())
    assert (0.4 if per_channel else 0.7) * ratio < got_ratio < 1.1 * ratio, got_ratio
    ref = torch.nn.functional.conv2d(torch.nn.functional.silu(torch.nn.functional.group_norm(y64, 32, host[0], host[1], norm.eps)),
                                     host[2], host[3], padding=1)
    calls = []
    orig = ops.call

    def counting(name, *a):
        calls.append(name)
        return orig(name, *a)
    ops.call = counting
    try:
        with torch.no_grad():
            z1 = norm_act_conv(norm_d, conv2_d, y1)                 # the registered moments
            n_stats = calls.count('mvip_groupnorm_stats')
            assert ops._LAST_Y[0] is None or ops._LAST_Y[0][0] is not y1
            z0 = norm_act_conv(norm_d, conv2_d, y1)                 # registration consumed: the pass over y
    finally:
        ops.call = orig
    assert n_stats == 0 and calls.count('mvip_groupnorm_stats') == 1, calls
    scale = float(ref.abs().max())
    e1 = float((z1.cpu().double() - ref).abs().max()) / scale
    e0 = float((z0.cpu().double() - ref).abs().max()) / scale
    print(f'tile moments {(N_, cin, cout, H, W)} mean/std {got_ratio:.1f} per_channel={per_channel}: '
          f'registered {e1:.3e}, two-pass {e0:.3e} of max |z|')
    assert e1 <= max(4.0 * e0, 3e-6), (e1, e0)


def test_groupnorm_planes_from_moment_partials(cuda):
    """mvip_groupnorm_split_planes_moments (statistics reduced inside the plane writer) writes the same bytes as
    mvip_groupnorm_stats + mvip_groupnorm_split_planes, for group sizes that do and do not divide 16."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.ops import call, ptr, stream
    for (N_, C, H, W, G) in [(2, 320, 16, 16, 32), (1, 128, 72, 64, 32), (2, 960, 8, 32, 32), (1, 640, 32, 32, 32)]:
        g = torch.Generator(device=cuda).manual_seed(C + H)
        x = torch.randn(N_, C, H, W, device=cuda, generator=g) * 2 + 0.5
        gw = torch.randn(C, device=cuda, generator=g)
        gb = torch.randn(C, device=cuda, generator=g)
        HW = H * W
        ws = ops._gn_workspace(N_, C, HW, cuda)
        mean = torch.empty((N_, G), device=cuda)
        rstd = torch.empty_like(mean)
        a = torch.zeros(N_ * C * HW * 2, device=cuda, dtype=torch.float16)
        b = torch.zeros_like(a)
        call('mvip_groupnorm_stats', ptr(x), N_, C, HW, G, 1e-5, 0, ptr(mean), ptr(rstd), ptr(ws, torch.float64), stream())
        call('mvip_groupnorm_split_planes', ptr(x), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N_, C, HW, G, 1,
             ptr(a, torch.float16), 0, stream())
        ws2 = torch.zeros_like(ws)
        call('mvip_groupnorm_stats', ptr(x), N_, C, HW, G, 1e-5, 0, None, None, ptr(ws2, torch.float64), stream())
        call('mvip_groupnorm_split_planes_moments', ptr(x), ptr(gw), ptr(gb), ptr(ws2, torch.float64), 1e-5, N_, C, HW, G, 1,
             ptr(b, torch.float16), 0, stream())
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (N_, C, H, W)


def test_gemm_f16x3(cuda):
    """Y = A X on the split-precision GEMM with strided operand sources vs fp64; tiny-magnitude operands (the
    gradients of the SDS step are ~1e-6) keep fp32-grade accuracy through the power-of-two scaling."""
    from mvip_nerf_amd import ops
    g = torch.Generator().manual_seed(0)
    M, K, P = 96, 64, 512
    A = torch.randn(M, K, generator=g) * 3e-6
    X = torch.randn(2, K, P, generator=g) * 2e-5
    bias, res = torch.randn(M, generator=g) * 1e-10, torch.randn(2, M, P, generator=g) * 1e-10
    ref = torch.einsum('mk,nkp->nmp', A.double(), X.double()) + bias.double()[None, :, None] + res.double()
    Xd = X.to(cuda)
    s2 = ops.absmax_scale(Xd)
    xs = ops.split_planes_strided(Xd, 2, K, P, K * P, P, 1, s2)
    y = ops.gemm_f16x3(xs, ops.gemm_pack_a(A.to(cuda), M, K, K, 1), 2, K, M, P, bias=bias.to(cuda),
                       residual=res.to(cuda), x_scale2=s2)
    np.testing.assert_allclose(N(y), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()))
    # transposed sources: A given as [K, M], X given as [P, K]
    At, Xt = A.T.contiguous().to(cuda), X[0].T.contiguous().to(cuda)
    xs = ops.split_planes_strided(Xt, 1, K, P, 0, 1, K, None)
    y2 = ops.gemm_f16x3(xs, ops.gemm_pack_a(At, M, K, 1, M), 1, K, M, P)
    ref2 = A.double() @ X[0].double()
    np.testing.assert_allclose(N(y2[0]), ref2.float().numpy(), rtol=0, atol=1e-3 * float(ref2.abs().max()))
    # a long contraction on a small grid: the library splits K over workgroups (1280-channel blocks at 16 x 16)
    M, K, P = 160, 1376, 256
    assert ops._lib.load().mvip_gemm_workspace_bytes(2, K, M, P) > 0
    A = torch.randn(M, K, generator=g) * 0.05
    X = torch.randn(2, K, P, generator=g)
    bias, ca = torch.randn(M, generator=g), torch.randn(2, M, generator=g)
    res = torch.randn(2, M, P, generator=g)
    ref = (torch.einsum('mk,nkp->nmp', A.double(), X.double()) + bias.double()[None, :, None] + ca.double()[:, :, None]
           + res.double())
    Xd = X.to(cuda)
    s2 = ops.absmax_scale(Xd)
    xs = ops.split_planes_strided(Xd, 2, K, P, K * P, P, 1, s2)
    y = ops.gemm_f16x3(xs, ops.gemm_pack_a(A.to(cuda), M, K, K, 1), 2, K, M, P, bias=bias.to(cuda), chan_add=ca.to(cuda),
                       residual=res.to(cuda), x_scale2=s2)
    np.testing.assert_allclose(N(y), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()))


def test_vae_attention_vs_fp64(cuda):
    from mvip_nerf_amd.guidance.sd_nets import VAEAttention
    from mvip_nerf_amd import ops
    torch.manual_seed(1)
    att = VAEAttention(64)
    att.requires_grad_(False)
    x = torch.randn(1, 64, 16, 32) * 1.5
    dy = torch.randn(1, 64, 16, 32) * 1e-5
    xr = x.double().requires_grad_(True)
    ref = att.double()(xr)
    ref.backward(dy.double())
    att_d = att.float().to(cuda)
    xd = x.to(cuda).requires_grad_(True)
    assert ops.vae_attention_supported(xd)
    y = att_d(xd)
    np.testing.assert_allclose(N(y), ref.detach().float().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))
    y.backward(dy.to(cuda))
    np.testing.assert_allclose(N(xd.grad), xr.grad.float().numpy(), rtol=0, atol=2e-5 * float(xr.grad.abs().max()))


def test_conv1x1_paths_vs_library(cuda):
    """1x1 convolutions on the split-precision GEMM (ResNet shortcut with gradient; transformer proj_in with
    GroupNorm; proj_out from token-major activations + residual) against the library convolution."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm
    torch.manual_seed(4)
    conv = torch.nn.Conv2d(64, 96, 1).to(cuda).requires_grad_(False)
    norm = GroupNorm(32, 64, eps=1e-6).to(cuda).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(64) + 0.5); norm.bias.copy_(torch.randn(64) * 0.2)
    x = torch.randn(2, 64, 16, 32, device=cuda)
    assert ops.conv1x1_supported(conv, x)
    xr = x.clone().requires_grad_(True)
    xd = x.clone().requires_grad_(True)
    dy = torch.randn(2, 96, 16, 32, device=cuda) * 1e-5
    ref = conv(xr); ref.backward(dy)
    got = ops.conv1x1(xd, conv); got.backward(dy)
    np.testing.assert_allclose(N(got), N(ref), rtol=0, atol=2e-5 * float(ref.abs().max()))
    np.testing.assert_allclose(N(xd.grad), N(xr.grad), rtol=0, atol=2e-5 * float(xr.grad.abs().max()))
    with torch.no_grad():
        ref = conv(torch.nn.functional.group_norm(x, 32, norm.weight, norm.bias, 1e-6))
        got = ops.norm_conv1x1(x, norm, conv).reshape(2, 96, 16, 32)
        np.testing.assert_allclose(N(got), N(ref), rtol=0, atol=2e-5 * float(ref.abs().max()))
        conv2 = torch.nn.Conv2d(96, 64, 1).to(cuda).requires_grad_(False)
        h = torch.randn(2, 512, 96, device=cuda)
        ref = x + conv2(h.reshape(2, 16, 32, 96).permute(0, 3, 1, 2))
        got = ops.tokens_conv1x1(h, conv2, x)
        np.testing.assert_allclose(N(got), N(ref), rtol=0, atol=2e-5 * float(ref.abs().max()))


def test_graphed_step_with_device_rng_and_host_churn(golden, cuda):
    """The graphed step with its own (device-side, replayed) random draws: every replay must give a gradient of the
    eager magnitude -- the step scalars once travelled in an asynchronous copy from a temporary host tensor and
    sporadically arrived as garbage when the host allocator reused the memory between steps."""
    g = golden('sds_rgb_i100')
    mags = {}
    for mode in (False, True):
        sd = make_sd(cuda, 0, 0)
        if '_randn' in sd.__dict__:
            del sd._randn                                 # the class's own generator-backed draws, not the recorded ones
        sd.use_graphs = mode
        torch.cuda.manual_seed(11)
        out = []
        busy = torch.randn(8192, 8192, device=cuda)
        mask_d = T(g['mask'], cuda)
        for i in range(100, 112):
            pred = T(g['pred'], cuda).requires_grad_(True)
            for _ in range(3):
                busy @ busy                                # keep the stream behind the host
            loss = sd.train_step_sd(i, mask_d, 'a stone bench in a park', pred, guidance_scale=7.5)
            junk = [torch.tensor([float(k), 1.0, 2.0, 3.0]) for k in range(64)]      # host allocator churn
            loss.sum().backward()
            out.append(float(pred.grad.abs().max()))
            del junk
        mags[mode] = np.array(out)
    assert np.all(np.isfinite(mags[True])) and np.all(mags[True] > 0)
    ratio = mags[True] / np.median(mags[False])
    assert ratio.min() > 0.3 and ratio.max() < 3.0, (mags[False], mags[True])


def test_graphed_full_size_step_is_replay_stable(cuda):
    """Full-size networks through the hand-written convolution / GroupNorm / attention kernels inside ONE captured
    hipGraph: replays with the same generator state must reproduce each other (and the eager step) -- a 16-byte
    hipMemsetAsync node in front of the data-gradient absmax reduction once left stale scales on replay and the
    gradient drifted from replay to replay (csrc/common.h::zero_words)."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False, use_graphs=True)
    gen = torch.Generator(device=cuda).manual_seed(2)
    pred = torch.rand(1, 3, 378, 504, device=cuda, generator=gen).requires_grad_(True)
    mask = torch.zeros(1, 1, 378, 504, device=cuda)
    mask[:, :, 137:241, 196:307] = 1

    def series(graphs, n=4):
        sd.use_graphs = graphs
        torch.cuda.manual_seed(77)
        out = []
        for k in range(n):
            pred.grad = None
            (1e-4 * sd.train_step_sd(1000 + k, mask, 'a stone bench in a park', pred, guidance_scale=7.5)).sum().backward()
            out.append(pred.grad.clone())
        return out

    first = series(True)                                    # capture (generator state restored afterwards) + first replays
    a, b, c = series(True), series(True), series(False)
    for w, x, y, z in zip(first, a, b, c):
        assert float((x - y).norm() / x.norm()) < 1e-4       # replay vs replay: atomics order only
        # vs eager: the SAME draws in the same order (tools/graph_vs_eager_draws.py: equal draw for draw), so atomics-level too
        assert float((x - z).norm() / z.norm()) < 1e-4
        # and the very first graphed call -- warm-up and capture draw as well, the generator state is put back -- likewise
        assert float((w - z).norm() / z.norm()) < 1e-4


def test_graphed_colla_step_equals_eager(cuda):
    """train_step_colla_sds as hipGraph replays (non-final views: forward-only 'share' graphs adding to the running latent
    gradient; final view: the 'last' graph that also carries the backward to the image, with the CFG-duplicated mask summed as
    SpecifyGradient's autograd does) against the eager method, same draws: the gradient of the stacked neighbour views is zero for
    every view but the last and equal there; also the sharded entry points colla_view_share / colla_last_view_image_grad."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False, use_graphs=True)
    gen = torch.Generator(device=cuda).manual_seed(5)
    NN, H, W = 3, 96, 128
    preds = torch.rand(NN, 3, H, W, device=cuda, generator=gen)
    masks = torch.zeros(NN, 1, H, W, device=cuda)
    masks[:, :, 30:70, 40:100] = 1
    out = {}
    for graphs in (True, False, True):
        sd.use_graphs = graphs
        torch.cuda.manual_seed(123)
        x = preds.clone().requires_grad_(True)
        loss = sd.train_step_colla_sds(0, masks, 'a stone bench in a park', x, guidance_scale=7.5)
        (1e-4 * loss).sum().backward()
        out.setdefault(graphs, []).append(x.grad.clone())
    ge, g1, g2 = out[False][0], out[True][0], out[True][1]
    assert float(ge[:NN - 1].abs().max()) == 0.0 and float(g1[:NN - 1].abs().max()) == 0.0     # only the last view receives gradient
    assert float(ge[NN - 1].abs().max()) > 0
    assert float((g1 - ge).norm() / ge.norm()) < 1e-4 and float((g2 - ge).norm() / ge.norm()) < 1e-4
    assert sorted(k[0] for k in sd._graphs) == ['last', 'share']                               # one graph per role, reused over the views
    # the per-term entry points of the view-sharded path, graphs vs eager
    res = {}
    for graphs in (True, False):
        sd.use_graphs = graphs
        shares = [sd.colla_view_share(k, masks[k:k + 1], 'a stone bench in a park', preds[k:k + 1], 7.5, seed=1000 + k) for k in range(NN - 1)]
        d = sd.colla_last_view_image_grad(NN - 1, masks[NN - 1:], 'a stone bench in a park', preds[NN - 1:], 7.5, sum(shares), weight=1e-4,
                                          seed=1000 + NN - 1)
        res[graphs] = (torch.stack(shares), d)
    sd.generator = None
    assert float((res[True][0] - res[False][0]).norm() / res[False][0].norm()) < 1e-4
    assert float((res[True][1] - res[False][1]).norm() / res[False][1].norm()) < 1e-4


def test_graphed_steps_with_two_alternating_prompts(cuda):
    """configs[2]/[3] alternate the RGB prompt and `text_normal` inside one iteration.  Each prompt's cross-attention
    key / value planes are cached per transformer (guidance/transformer_cm.py::_prompt_kv) and a captured hipGraph
    replays against the addresses of the entry it was captured with: the cache must keep BOTH prompts' entries alive
    (it once held one prompt and freed the other's planes under the other graph).  Graph replays of A, B, A, B must
    equal the eager steps of the same prompts with the same draws, and the cache must hold both prompts."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    from mvip_nerf_amd.guidance import transformer_cm
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False)
    gen = torch.Generator(device=cuda).manual_seed(4)
    pred = torch.rand(1, 3, 96, 128, device=cuda, generator=gen).requires_grad_(True)
    mask = torch.zeros(1, 1, 96, 128, device=cuda)
    mask[:, :, 30:70, 40:90] = 1
    prompts = ('a stone bench in a park', 'a normal map of a stone bench in a park')

    def series(graphs):
        sd.use_graphs = graphs
        out = []
        for k in range(6):
            torch.cuda.manual_seed(100 + k)
            pred.grad = None
            (1e-4 * sd.train_step_sd(1000 + 37 * k, mask, prompts[k % 2], pred, guidance_scale=7.5)).sum().backward()
            out.append(pred.grad.clone())
            if graphs and k == 1:                   # between replays: churn the allocator so that freed planes WOULD be reused
                junk = [torch.randn(1 << 18, device=cuda) for _ in range(64)]
                del junk
        return out

    eager = series(False)
    series(True)                                    # captures one graph per prompt
    assert len(sd._graphs) == 2
    graphed = series(True)
    for k, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.isfinite(b).all()
        assert float((a - b).norm() / a.norm()) < 1e-4, k        # same draws, same order: atomics-level
    assert float((eager[0] - eager[1]).norm() / eager[0].norm()) > 1e-3        # the prompts really differ
    for m in sd.unet.modules():
        pk = m.__dict__.get('_mvip_cm')
        if pk is not None:
            assert len(pk.ctx_cache) == 2
    assert all(len(g.pinned) >= 16 for g in sd._graphs.values())
    assert len(transformer_cm.prompt_entries(sd.unet)) == 32


@pytest.mark.parametrize('N_,cin,cout,H,W', [(2, 320, 64, 8, 8), (2, 640, 64, 16, 16), (1, 256, 32, 8, 32)])
def test_conv3x3_with_and_without_workspace(cuda, N_, cin, cout, H, W):
    """mvip_conv3x3_f16x3 (no workspace: one workgroup contracts all input channels) and mvip_conv3x3_f16x3_ws (channel
    splits + ordered reduction) through the C ABI on the same operands: equal up to fp32 summation order, and the split
    path is bit-reproducible."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd._lib import ptr, stream, call
    g = torch.Generator().manual_seed(N_ + cin + H)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(cuda)
    for p_ in conv.parameters():
        p_.requires_grad_(False)
    x = torch.randn(N_, cin, H, W, generator=g).to(cuda)
    rs = torch.randn(N_, cout, H, W, generator=g).to(cuda)
    ca = torch.randn(N_, cout, generator=g).to(cuda)
    s2 = ops.absmax_scale(x)
    xs = ops._split_buffer(N_, cin, H * W, cuda)
    call('mvip_split_planes', ptr(x), N_, cin, H * W, ptr(s2), ptr(xs, torch.float16), 0, stream())
    pk = ops._conv_packed(conv, False)
    bias = conv.bias.detach()
    nbytes = int(_lib.load().mvip_conv3x3_workspace_bytes(N_, cin, cout, H, W))
    assert nbytes > 0
    ws = torch.empty(nbytes // 4, device=cuda)
    y0, y1, y2 = (torch.empty(N_, cout, H, W, device=cuda) for _ in range(3))
    call('mvip_conv3x3_f16x3', ptr(xs, torch.float16), ptr(pk, torch.uint8), ptr(bias), ptr(ca), ptr(rs), ptr(s2), N_, cin, cout,
         H, W, ptr(y0), 0, stream())
    for y in (y1, y2):
        call('mvip_conv3x3_f16x3_ws', ptr(xs, torch.float16), ptr(pk, torch.uint8), ptr(bias), ptr(ca), ptr(rs), ptr(s2), N_,
             cin, cout, H, W, ptr(y), ptr(ws), 0, stream())
    ref = torch.nn.functional.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1) + ca.double()[:, :, None, None] + rs.double()
    scale = float(ref.abs().max())
    np.testing.assert_allclose(N(y0), ref.float().cpu().numpy(), rtol=0, atol=1e-5 * scale)
    np.testing.assert_allclose(N(y1), N(y0), rtol=0, atol=2e-6 * scale)
    assert torch.equal(y1, y2)
    with pytest.raises(Exception):                           # the library refuses a missing workspace where it needs one
        call('mvip_conv3x3_f16x3_ws', ptr(xs, torch.float16), ptr(pk, torch.uint8), ptr(bias), ptr(ca), ptr(rs), ptr(s2), N_,
             cin, cout, H, W, ptr(y1), ptr(None), 0, stream())


@pytest.mark.parametrize('fp16', [False, True])
def test_sds_step_launches_no_library_contraction(cuda, fp16):
    """(fp16 = True: the reference's --fp16 mode, DS_NeRF/guidance/sd_utils.py:66 -- the same hand-written kernels in their
    single-product instantiations; it used to fall through every dtype gate onto MIOpen / CK / AOTriton.)
    One full-size train_step_sd (forward + backward to the image) under the profiler: no library convolution, GEMM,
    attention or layout-transpose kernel is launched -- every contraction of the step is a kernel of this repository
    (MIOpen: `igemm`, `miopen`, `naive_conv`, `Im2d2Col`, `Col2Im`, `batched_transpose`; hipBLASLt / rocBLAS: `Cijk_`;
    AOTriton: `attn_fwd`)."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, fp16, False)
    assert sd.unet.mfma_prec == int(fp16) and sd.vae.mfma_prec == int(fp16)
    assert sd.use_graphs is True               # the built-in networks replay a captured hipGraph by default ...
    sd.use_graphs = False                      # ... this test wants to see the launches one by one
    gen = torch.Generator(device=cuda).manual_seed(3)
    pred = torch.rand(1, 3, 378, 504, device=cuda, generator=gen).requires_grad_(True)
    mask = torch.zeros(1, 1, 378, 504, device=cuda)
    mask[:, :, 137:241, 196:307] = 1

    def step(i):
        pred.grad = None
        (1e-4 * sd.train_step_sd(i, mask, 'a stone bench in a park', pred, guidance_scale=7.5)).sum().backward()
    step(1000)                                               # packs weights, caches the prompt embedding
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step(1001)
        torch.cuda.synchronize()
    assert torch.isfinite(pred.grad).all() and float(pred.grad.abs().max()) > 0
    names = [e.key for e in prof.key_averages()]
    banned = ('igemm', 'miopen', 'naive_conv', 'Im2d2Col', 'Col2Im', 'batched_transpose', 'Cijk_', 'attn_fwd', 'ck::',
              'grouped_conv', 'MIOpen', 'gemm_kernel', 'softmax_warp', 'SoftMax', 'upsample_nearest')
    assert not [n for n in names if any(b in n for b in banned)], [n for n in names if any(b in n for b in banned)]
    for must in ('conv3x3_f16x3_kernel', 'gemm5_f16x3_kernel', 'attn_f16x3_kernel', 'cv_im2col_split_kernel',
                 'resize_bilinear_fwd_kernel', 'resize_bilinear_bwd_kernel'):
        assert any(must in n for n in names), must
    # the number of products per contraction step shows in the kernel names: the last template argument of the convolution
    # / GEMM kernels (1 = fp16 mode, 2 = two products on fp16-exact weights, 3 = three), <..., true> of the attention kernel
    def last_arg(n):
        return n.split('(')[0].rstrip('>').split(',')[-1].strip()
    wk = [n for n in names if 'conv3x3_f16x3_kernel' in n or 'gemm5_f16x3_kernel' in n]
    at = [n for n in names if 'attn_f16x3_kernel' in n]
    if fp16:
        assert all(last_arg(n) == '1' for n in wk), wk
        assert all(last_arg(n) == 'true' for n in at), at
    else:
        assert all(last_arg(n) == 'false' for n in at), at
        # the built-in networks' weights are fp16-representable like the reference's (revision="fp16" cast up): every
        # convolution and every weight GEMM runs TWO products; three only where an ACTIVATION is the packed operand (the VAE
        # mid-block attention's products)
        assert sd.networks.fp16_weights
        assert all(last_arg(n) in ('2', '3') for n in wk), wk
        assert all(last_arg(n) == '2' for n in wk if 'conv3x3_f16x3_kernel' in n), wk
        assert any(last_arg(n) == '2' for n in wk if 'gemm5_f16x3_kernel' in n), wk


def test_plain_conv3x3_on_mfma_kernel(cuda):
    """ops.conv3x3_plain (no GroupNorm in front: the UNet's up-sampling convolutions) vs the same convolution in fp64;
    inputs of very different magnitude exercise the power-of-two input scale."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import Upsample2D
    gen = torch.Generator().manual_seed(5)
    for mag in (1e-4, 1.0, 300.0):
        up = Upsample2D(64)
        with torch.no_grad():
            up.conv.weight.copy_(torch.randn(up.conv.weight.shape, generator=gen) * 0.06)
            up.conv.bias.copy_(torch.randn(64, generator=gen) * 0.1 * mag)
        x = torch.randn(2, 64, 8, 16, generator=gen) * mag
        ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x.double(), scale_factor=2.0, mode='nearest'),
                                         up.conv.weight.double(), up.conv.bias.double(), padding=1)
        up = up.to(cuda)
        with torch.no_grad():
            assert ops.conv3x3_supported(up.conv, torch.empty(2, 64, 16, 32, device=cuda))
            got = up(x.to(cuda))
        np.testing.assert_allclose(N(got), ref.detach().float().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))
    # with autograd enabled on a grad-carrying input the module takes a differentiable path (ops.conv_gemm)
    xg = torch.randn(1, 64, 8, 16, device=cuda, requires_grad=True)
    assert up(xg).requires_grad


def test_fp16_mode_kernels_vs_fp64(cuda):
    """ops.precision(1) -- the reference's --fp16 arithmetic on the hand-written kernels: ONE fp16 product per step, fp32
    accumulate, hi planes only -- against fp64 at fp16 tolerance (2e-3 of the output scale), forward and data gradient of
    the GroupNorm + SiLU + 3x3 convolution, the GEMM (incl. split-K) and the im2col convolution; and it really IS the
    single-product path (error well above the split-precision kernels' 1e-5)."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import GroupNorm, norm_act_conv
    gen = torch.Generator().manual_seed(12)
    for N_, cin, cout, H, W in ((1, 128, 128, 32, 32), (2, 320, 64, 8, 8), (2, 640, 64, 16, 16), (1, 64, 64, 8, 64)):
        norm = GroupNorm(32, cin, eps=1e-6)
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_((torch.randn(conv.weight.shape, generator=gen) * (2.0 / (9 * cin)) ** 0.5).half().float())
        for p in list(norm.parameters()) + list(conv.parameters()):
            p.requires_grad_(False)
        x = torch.randn(N_, cin, H, W, generator=gen) * 1.3 + 0.2
        dy = torch.randn(N_, cout, H, W, generator=gen) * 1e-5
        xr = x.double().requires_grad_(True)
        h = torch.nn.functional.silu(torch.nn.functional.group_norm(xr, 32, norm.weight.double(), norm.bias.double(), 1e-6))
        yr = torch.nn.functional.conv2d(h, conv.weight.double(), conv.bias.double(), padding=1)
        yr.backward(dy.double())
        norm_d, conv_d = norm.to(cuda), conv.to(cuda)
        xd = x.to(cuda).requires_grad_(True)
        with ops.precision(1):
            y = norm_act_conv(norm_d, conv_d, xd)
        y.backward(dy.to(cuda))                                  # outside the context: the Function remembers its arithmetic
        e_f = float((y.detach().cpu().double() - yr.detach()).abs().max() / yr.abs().max())
        e_b = float((xd.grad.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max())
        assert 2e-5 < e_f < 2e-3 and e_b < 2e-3, (cin, cout, H, W, e_f, e_b)
    # GEMM, also split over K
    for M, K, P in ((96, 64, 512), (160, 1376, 256)):
        A = (torch.randn(M, K, generator=gen) * 0.05).half().float()
        X = torch.randn(2, K, P, generator=gen)
        bias, res = torch.randn(M, generator=gen), torch.randn(2, M, P, generator=gen)
        ref = torch.einsum('mk,nkp->nmp', A.double(), X.double()) + bias.double()[None, :, None] + res.double()
        Xd = X.to(cuda)
        with ops.precision(1):
            s2 = ops.absmax_scale(Xd)
            xs = ops.split_planes_strided(Xd, 2, K, P, K * P, P, 1, s2)
            y = ops.gemm_f16x3(xs, ops.gemm_pack_a(A.to(cuda), M, K, K, 1), 2, K, M, P, bias=bias.to(cuda), residual=res.to(cuda),
                               x_scale2=s2)
        err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
        assert 2e-6 < err < 2e-3, (M, K, P, err)
    # stride-2 convolution through im2col planes + GEMM, forward and data gradient
    conv = torch.nn.Conv2d(128, 128, 3, stride=2, padding=1)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.half().float())
    for p in conv.parameters():
        p.requires_grad_(False)
    x = torch.randn(1, 128, 32, 32, generator=gen)
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, conv.weight.double(), conv.bias.double(), stride=2, padding=1)
    yr.sum().backward()
    xd = x.to(cuda).requires_grad_(True)
    with ops.precision(1):
        y = ops.conv_gemm(xd, conv.to(cuda))
    y.sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max() / yr.abs().max()) < 2e-3
    assert float((xd.grad.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max()) < 2e-3


def test_softmax_rows_and_upsample_fold(cuda):
    """The last stock torch compute ops of the SDS step, replaced: the VAE mid-block attention's row softmax
    and its adjoint (csrc/sds_elem.hip) vs fp64, and the nearest-neighbour up-sampling folded into the plane writer vs the
    materialised F.interpolate + convolution (bit-identical: the same values reach the same kernel)."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_nets import Upsample2D
    gen = torch.Generator().manual_seed(9)
    for rows, cols in ((64, 4096), (7, 1000), (3, 8192), (5, 1)):
        S = torch.randn(rows, cols, generator=gen) * 40.0
        dP = torch.randn(rows, cols, generator=gen)
        Sr = S.double().requires_grad_(True)
        Pr = torch.softmax(Sr * 0.044, -1)
        (Pr * dP.double()).sum().backward()
        P = ops.softmax_rows(S.to(cuda), 0.044)
        np.testing.assert_allclose(N(P), Pr.detach().float().numpy(), rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(N(P.sum(-1)), np.ones(rows, np.float32), rtol=0, atol=2e-6)
        dS = ops.softmax_rows_backward(P, dP.to(cuda), 0.044)
        np.testing.assert_allclose(N(dS), Sr.grad.float().numpy(), rtol=0, atol=3e-6 * float(Sr.grad.abs().max()))
    up = Upsample2D(64).to(cuda)
    for p in up.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 64, 8, 16, generator=gen).to(cuda)
    with torch.no_grad():
        folded = up(x)
        xi = torch.nn.functional.interpolate(x, scale_factor=2.0, mode='nearest')
        mat = ops.conv3x3_plain(xi, up.conv)
    assert folded.shape == (2, 64, 16, 32) and torch.equal(folded, mat)


def test_fp16_mode_step_agrees_with_fp32_mode(cuda):
    """The reference's --fp16 step and its fp32 step compute the same function at different precision: with the SAME
    (fp16-representable) weights and the same noise, the image gradient of the single-product kernels agrees with the one of
    the split-precision kernels to fp16 grade through ~60 chained layers (measured: relative L2 difference 3.8e-2, cosine
    0.9993; asserted < 8e-2, > 0.997)."""
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    torch.manual_seed(0)
    sd16 = StableDiffusion(cuda, True, False, use_graphs=False)
    sd32 = StableDiffusion(cuda, False, False, use_graphs=False)
    for m16, m32 in ((sd16.vae, sd32.vae), (sd16.unet, sd32.unet), (sd16.networks.text_encoder, sd32.networks.text_encoder)):
        m32.load_state_dict(m16.state_dict())                  # the fp16-rounded values, in both
    gen = torch.Generator(device=cuda).manual_seed(6)
    pred0 = torch.rand(1, 3, 378, 504, device=cuda, generator=gen)
    mask = torch.zeros(1, 1, 378, 504, device=cuda)
    mask[:, :, 137:241, 196:307] = 1
    grads = []
    for sd in (sd32, sd16):
        torch.cuda.manual_seed(21)
        pred = pred0.clone().requires_grad_(True)
        (1e-4 * sd.train_step_sd(1500, mask, 'a stone bench in a park', pred, guidance_scale=7.5)).sum().backward()
        assert torch.isfinite(pred.grad).all() and float(pred.grad.abs().max()) > 0
        grads.append(pred.grad.double().flatten())
    a, b = grads
    rel = float((a - b).norm() / a.norm())
    cos = float((a @ b) / (a.norm() * b.norm()))
    print(f'fp16-mode vs fp32-mode SDS image gradient: relative L2 {rel:.3e}, cosine {cos:.6f}')
    assert rel < 8e-2 and cos > 0.997, (rel, cos)


def _fp16_exact(t):
    return t.half().float()


@pytest.mark.parametrize('N_,cin,cout,H,W', [(1, 128, 128, 64, 64), (2, 320, 320, 16, 16), (2, 1280, 640, 8, 8), (1, 64, 32, 8, 32)])
def test_two_product_convolution_equals_three_product(cuda, N_, cin, cout, H, W):
    """prec = 2 (csrc/conv3x3.hip NP = 2: W_hi x_hi + W_hi x_lo, the weights' lo fragments neither fetched nor multiplied)
    against prec = 0 on weights that are exact fp16 values, as every weight the reference loads is
    (DS_NeRF/guidance/sd_utils.py:69-74): EQUAL outputs (the third product adds exact zeros), every tile shape (32 / 16 / 8
    wide, channel-split or not), forward and transposed operator; the packer reports the image as two-product capable, and
    says no for a weight with a non-zero lo half."""
    from mvip_nerf_amd import ops, _lib
    from mvip_nerf_amd._lib import ptr, stream, call
    g = torch.Generator().manual_seed(cin + H)
    w = _fp16_exact(torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(cuda)
    x = torch.randn(N_, cin, H, W, generator=g).to(cuda)
    bias = torch.randn(cout, generator=g).to(cuda)
    s2 = ops.absmax_scale(x)
    xs = ops._split_buffer(N_, cin, H * W, cuda)
    call('mvip_split_planes', ptr(x), N_, cin, H * W, ptr(s2), ptr(xs, torch.float16), 0, stream())
    for transpose in (False, True):
        pk = ops.conv3x3_pack(w if not transpose else w.permute(1, 0, 2, 3).contiguous(), transpose)
        assert pk._mvip_two_product is True
        nbytes = int(_lib.load().mvip_conv3x3_workspace_bytes(N_, cin, cout, H, W))
        ws = torch.empty(max(nbytes // 4, 1), device=cuda)
        ys = []
        for prec in (0, 2):
            y = torch.empty(N_, cout, H, W, device=cuda)
            call('mvip_conv3x3_f16x3_ws', ptr(xs, torch.float16), ptr(pk, torch.uint8), ptr(bias), None, None, ptr(s2), N_, cin,
                 cout, H, W, ptr(y), ptr(ws), prec, stream())
            ys.append(y)
        assert torch.equal(ys[0], ys[1])
    ref = torch.nn.functional.conv2d(x.double(), w.double(), bias.double(), padding=1)
    pk = ops.conv3x3_pack(w, False)
    y = torch.empty(N_, cout, H, W, device=cuda)
    call('mvip_conv3x3_f16x3', ptr(xs, torch.float16), ptr(pk, torch.uint8), ptr(bias), None, None, ptr(s2), N_, cin, cout, H, W,
         ptr(y), 2, stream())
    np.testing.assert_allclose(N(y), ref.float().cpu().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))
    w_full = (w + torch.randn(w.shape, generator=g).to(cuda) * 1e-6)
    assert ops.conv3x3_pack(w_full, False)._mvip_two_product is False


def test_two_product_gemm_paths_equal_three_product(cuda):
    """The weight GEMMs in their two-product instantiations (gemm5 NP = 2: plain, split-K, GEGLU epilogue, operand sinks incl.
    the transposed V-fragment launch) equal the three-product ones bit for bit on fp16-exact weights."""
    from mvip_nerf_amd import ops
    g = torch.Generator().manual_seed(11)
    for (N_, K, M, P) in ((2, 320, 320, 4096), (2, 1280, 1280, 256), (1, 640, 64, 1024)):
        w = _fp16_exact(torch.randn(M, K, generator=g) * 0.04).to(cuda)
        x = torch.randn(N_, K, P, generator=g).to(cuda)
        b = torch.randn(M, generator=g).to(cuda)
        pk = ops.gemm_pack_a(w, M, K, K, 1, weights=True)
        assert pk._mvip_two_product is True
        assert not hasattr(ops.gemm_pack_a(w, M, K, K, 1), '_mvip_two_product')       # activations packed per step never ask
        s2 = ops.absmax_scale(x)
        xs = ops.split_planes_strided(x, N_, K, P, K * P, P, 1, s2)
        outs = []
        for two in (False, True):
            ops.TWO_PRODUCT = two
            try:
                assert ops._prec_w(pk) == (2 if two else 0)
                outs.append(ops.gemm_f16x3(xs, pk, N_, K, M, P, bias=b, x_scale2=s2))
                if M % 64 == 0:
                    outs.append(ops.gemm_f16x3_planes(xs, pk, N_, K, M, P, 0.25, bias=b, x_scale2=s2))
            finally:
                ops.TWO_PRODUCT = True
        h = len(outs) // 2
        for a, c in zip(outs[:h], outs[h:]):
            assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, c.view(torch.int16) if c.dtype == torch.float16 else c)
        ref = torch.einsum('mk,nkp->nmp', w.double(), x.double()) + b.double()[None, :, None]
        np.testing.assert_allclose(N(outs[h]), ref.float().cpu().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))
    # a weight with a non-zero lo half keeps the three-product kernels
    w_full = torch.randn(64, 64, generator=g).to(cuda)
    pk = ops.gemm_pack_a(w_full, 64, 64, 64, 1, weights=True)
    assert pk._mvip_two_product is False and ops._prec_w(pk) == 0


def test_two_product_step_equals_three_product_step(cuda):
    """VERDICT r3 task 1(a): one full-size train_step_sd with the built-in networks (fp16-representable random weights, like
    the reference's revision="fp16" checkpoint cast up to fp32) run with two products per contraction step and with three:
    the image gradient is EQUAL (torch.equal; the third product adds exact zeros).  And the networks built with
    fp16_weights=False (full fp32 random values) never take the two-product kernels."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    from mvip_nerf_amd.guidance.sd_nets import SDNetworks
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False, use_graphs=False)
    assert sd.networks.fp16_weights
    for p_ in list(sd.unet.parameters())[:20] + list(sd.vae.parameters())[:20]:
        assert torch.equal(p_.half().float(), p_)
    mask = torch.zeros(1, 1, 378, 504, device=cuda)
    mask[:, :, 137:241, 196:307] = 1
    base = torch.rand(1, 3, 378, 504, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))
    grads = {}
    for two in (True, False, True):
        ops.TWO_PRODUCT = two
        try:
            sd.seed_generator(77)
            pred = base.clone().requires_grad_(True)
            (1e-4 * sd.train_step_sd(1000, mask, 'a stone bench in a park', pred, guidance_scale=7.5)).sum().backward()
            grads.setdefault(two, []).append(pred.grad.clone())
        finally:
            ops.TWO_PRODUCT = True
    assert torch.isfinite(grads[True][0]).all() and float(grads[True][0].abs().max()) > 0
    assert torch.equal(grads[True][0], grads[True][1])              # the step itself is reproducible
    assert torch.equal(grads[True][0], grads[False][0])             # ... and two products EQUAL three
    del sd
    torch.cuda.empty_cache()
    nets = SDNetworks(cuda, torch.float32, fp16_weights=False)
    conv = nets.vae.encoder.down_blocks[0].resnets[0].conv1
    assert ops._conv_packed(conv, False)._mvip_two_product is False


@pytest.mark.gpu
def test_posterior_sample_and_timestep_embedding_kernels(cuda):
    """csrc/sds_elem.hip: the one-launch posterior sample sf * (mean + exp(0.5 clamp(logvar)) * noise) with its adjoint, and the
    one-launch sinusoidal timestep embedding, against the torch expressions they replace (values AND gradients; logvar values
    beyond both clamp bounds included)."""
    from mvip_nerf_amd.guidance import sd_nets
    g = torch.Generator().manual_seed(21)
    m = torch.randn(2, 8, 16, 24, generator=g)
    m[0, 5, 0, :4] = torch.tensor([-31.0, 25.0, -30.0, 20.0])               # outside / on the clamp bounds
    noise = torch.randn(2, 4, 16, 24, generator=g)
    gout = torch.randn(2, 4, 16, 24, generator=g)
    md = m.to(cuda).requires_grad_(True)
    out = sd_nets.LatentDist(md).scaled_sample(noise.to(cuda), 0.18215)
    out.backward(gout.to(cuda))
    mr = m.clone().requires_grad_(True)
    mean, logvar = torch.chunk(mr, 2, dim=1)
    ref = 0.18215 * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)
    ref.backward(gout)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(md.grad.cpu().numpy(), mr.grad.numpy(), rtol=2e-6, atol=1e-9)
    assert float(md.grad[0, 5, 0, 0]) == 0.0 and float(md.grad[0, 5, 0, 1]) == 0.0       # clamped: no gradient to logvar
    # the lazily formed properties are diffusers' DiagonalGaussianDistribution fields
    d = sd_nets.LatentDist(m)
    assert torch.equal(d.mean, m[:, :4]) and torch.equal(d.std, torch.exp(0.5 * torch.clamp(m[:, 4:], -30.0, 20.0)))
    # timestep embedding: device kernel vs the host expression, integer and fractional timesteps
    for t in (torch.tensor([980.0, 20.0]), torch.tensor([501.25])):
        got = sd_nets.timestep_sinusoid(t.to(cuda), 320)
        half = 160
        # the expression it replaces, evaluated where the reference evaluates it (on the device: a host exp() differs from
        # the device's by an ulp in some frequencies, i.e. by 6e-5 in an argument of 980)
        freqs = torch.exp(-np.log(10000.0) * torch.arange(half, dtype=torch.float32, device=cuda) / half)
        args = t.to(cuda)[:, None].float() * freqs[None]
        ref = torch.cat([torch.cos(args), torch.sin(args)], -1)
        assert got.shape == (t.shape[0], 320)
        np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=5e-7)
        ref64 = torch.cat([torch.cos(args.double()), torch.sin(args.double())], -1)          # and against the exact functions
        np.testing.assert_allclose(got.cpu().numpy(), ref64.cpu().numpy(), rtol=0, atol=5e-7)


def test_concurrent_sds_terms_equal_sequential_terms(cuda):
    """Pretrain_Model.cal_loss (DS_NeRF/nerf/utils.py:280-302) with its terms on one stream each (round 5: the captured RGB /
    collaborative / normal steps replay side by side) against the same terms in line: same draws, the gradients with respect to
    the RGB frame, the normal map and the neighbour views are EQUAL (each graph owns its scratch words, ops.ZERO_SCOPE; the steps
    share nothing else that is written), three iterations in a row."""
    import types
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    from mvip_nerf_amd.nerf.utils import Pretrain_Model
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False, use_graphs=True)
    opt = types.SimpleNamespace(is_rgb_guidance=True, is_colla_guidance=True, is_normal_guidance=True, normal_start=0,
                                text='a stone bench in a park', text_normal='a normal map of a stone bench in a park',
                                rgb_guidance_scale=7.5, colla_guidance_scale=7.5, normal_guidance_scale=7.5, lambda_guidance=1.0,
                                uniform_sphere_rate=0.5)
    pm = Pretrain_Model(opt, cuda, {'SD': sd})
    gen = torch.Generator(device=cuda).manual_seed(9)
    H, W = 96, 128
    rgb0 = torch.rand(1, 3, H, W, device=cuda, generator=gen)
    nrm0 = torch.rand(1, 3, H // 2, W // 2, device=cuda, generator=gen)
    nb0 = torch.rand(2, 3, H // 2, W // 2, device=cuda, generator=gen)
    mask = torch.zeros(1, 1, H, W, device=cuda)
    mask[:, :, 30:70, 40:100] = 1
    mask4 = mask.expand(2, 1, H, W).contiguous()
    real_streams = pm._term_streams
    out = {}
    for mode in ('streams', 'in_line', 'streams'):
        pm._term_streams = real_streams if mode == 'streams' else (lambda sd_, n: None)
        import random
        random.seed(3)
        torch.cuda.manual_seed(321)
        grads = []
        for it in (5, 6, 7):
            rgb, nrm, nb = (t.clone().requires_grad_(True) for t in (rgb0, nrm0, nb0))
            loss = pm.cal_loss(it, nb, nrm, None, rgb, None, mask, mask4, 1)
            (1e-4 * loss).sum().backward()
            grads.append((rgb.grad.clone(), nrm.grad.clone(), nb.grad.clone()))
        out.setdefault(mode, []).append(grads)
    assert pm.__dict__.get('_streams') and len(pm._streams) == 3
    ref = out['in_line'][0]
    for run_ in out['streams']:
        for ga, gb in zip(run_, ref):
            for a, b in zip(ga, gb):
                assert float(b.abs().max()) > 0
                assert float((a - b).norm() / b.norm()) < 1e-4           # graph replays differ by fp32 atomics order only


def test_concurrent_terms_with_identical_prompt_scale_and_shape_do_not_share_a_graph(cuda):
    """the reference's defaults give the RGB and the normal term the SAME prompt (--text == --text_normal),
    the same guidance scale (7.5) and, with normalmap_render_factor = 1, the same shapes (DS_NeRF/nerf/utils.py:280-302); both use
    mode 'single'.  Replayed on one stream each they must not resolve to one captured graph (one set of static input / output
    buffers): the graph key carries the stream, and _GraphedStep.run waits for the previous run's clones.  Checked: one graph
    per stream exists, the gradients equal the in-line evaluation's for three iterations, and ONE graph driven from two streams
    back to back (the guard in run) equals the same two runs on one stream."""
    import random
    import types
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    from mvip_nerf_amd.nerf.utils import Pretrain_Model
    torch.manual_seed(0)
    sd = StableDiffusion(cuda, False, False, use_graphs=True)
    opt = types.SimpleNamespace(is_rgb_guidance=True, is_colla_guidance=False, is_normal_guidance=True, normal_start=0,
                                text='a stone bench in a park', text_normal='a stone bench in a park',
                                rgb_guidance_scale=7.5, colla_guidance_scale=7.5, normal_guidance_scale=7.5, lambda_guidance=1.0,
                                uniform_sphere_rate=0.5)
    pm = Pretrain_Model(opt, cuda, {'SD': sd})
    gen = torch.Generator(device=cuda).manual_seed(11)
    H, W = 96, 128
    rgb0 = torch.rand(1, 3, H, W, device=cuda, generator=gen)
    nrm0 = torch.rand(1, 3, H, W, device=cuda, generator=gen)
    mask = torch.zeros(1, 1, H, W, device=cuda)
    mask[:, :, 30:70, 40:100] = 1
    real_streams = pm._term_streams
    out = {}
    for mode in ('streams', 'in_line', 'streams'):
        pm._term_streams = real_streams if mode == 'streams' else (lambda sd_, n: None)
        random.seed(3)
        torch.cuda.manual_seed(321)
        grads = []
        for it in (5, 6, 7):
            rgb, nrm = (t.clone().requires_grad_(True) for t in (rgb0, nrm0))
            loss = pm.cal_loss(it, None, nrm, None, rgb, None, mask, None, 1)
            (1e-4 * loss).sum().backward()
            grads.append((rgb.grad.clone(), nrm.grad.clone()))
        out.setdefault(mode, []).append(grads)
    singles = [k for k in sd._graphs if k[0] == 'single']
    # term stream 0 and term stream 1: the in-line evaluation of this two-term model hops off the DEFAULT stream onto term stream 0
    # (sd_utils._OffDefaultStream in cal_loss), where its two terms share one graph -- one after the other, which is safe
    assert len(singles) == 2 and len({k[-1] for k in singles}) == 2
    ref = out['in_line'][0]
    for run_ in out['streams']:
        for ga, gb in zip(run_, ref):
            for a, b in zip(ga, gb):
                assert float(b.abs().max()) > 0
                assert float((a - b).norm() / b.norm()) < 1e-4
    # the two terms see different images: their gradients differ (a shared graph made them collide)
    assert float((ref[0][0] - ref[0][1]).norm() / ref[0][0].norm()) > 1e-2
    # the guard for callers that DO share a graph across streams: the same graph run from two streams back to back
    g = sd._graphs[singles[0]]
    s1, s2 = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    torch.cuda.manual_seed(5)
    with torch.cuda.stream(s1):
        a1 = g.run(rgb0, mask, 500)
    with torch.cuda.stream(s2):
        a2 = g.run(nrm0, mask, 500)
    torch.cuda.synchronize()
    torch.cuda.manual_seed(5)
    b1 = g.run(rgb0, mask, 500)
    b2 = g.run(nrm0, mask, 500)
    torch.cuda.synchronize()
    assert float((a1 - b1).norm() / b1.norm()) < 1e-4 and float((a2 - b2).norm() / b2.norm()) < 1e-4
    assert float((a1 - a2).norm() / a1.norm()) > 1e-2
