"""The SDS networks' COMPOSED HIP paths against the same sd_nets modules evaluated on the host in fp64 (their host branches
are plain torch ops): the whole UNet forward and the whole VAE encoder, forward and data gradient, at the smallest sizes at
which the hand-written kernels still run at every level.  Each kernel family (conv3x3.hip, group_norm.hip, attention.hip,
transformer.hip, the split-precision GEMM of gemm_f16x3.hip) is pinned on its own elsewhere; here a stale power-of-two scale, a plane handed
to the wrong consumer, a hit of the _LAST_Y / _LAST_DX registries on the wrong tensor, the 22 grouped time projections
handed to the wrong blocks, or an H / W transposition would show.

Weights (tests/sd_network_cases.py::seeded_network): seeded default initialisation, every GroupNorm / LayerNorm weight and
bias moved away from 1 / 0, frozen; once rounded to fp16 values (what SDNetworks ships: two-product kernels) and once as they
are (three-product kernels).  The fp64 twin holds the same values.

Bounds: per output max |got - ref| / max |ref| and |got - ref|_2 / |ref|_2, each 8x the largest value measured on an MI355X
over the cases that share it, rounded up to one significant digit, and never above the ceilings of the per-family tests (UNet
eps 2e-5: test_transformer2d_hip_path_vs_fp64_module's 1e-5 doubled for depth; encoder moments and image gradient 1e-4:
test_decode_latents_against_host_decoder; the single-product mode 5e-3: test_transformer2d_fp16_mode_vs_fp64).  The measured
values stand beside the bounds and in DESIGN.md section 6; every test prints its figures.  For comparison, the same modules in
fp32 on the HOST sit at 7.5e-7 (UNet, 32^2), 6.6e-7 (UNet, 64^2) and 1.0e-6 (encoder moments) of max |ref| from their twins."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sd_network_cases import errors, library_kernels_in, seeded_network            # noqa: E402

pytestmark = pytest.mark.gpu

# (bound on max |got - ref| / max |ref|, bound on the relative L2 error); measured (max, L2) beside each
UNET_BOUND = (9e-6, 8e-6)          # 64^2: 8.6e-7, 8.0e-7; 32^2 fp16 weights: 1.01e-6, 7.5e-7; 32^2 fp32 weights: 1.04e-6, 8.8e-7
UNET_FP16_BOUND = (5e-3, 5e-3)     # single product, 32^2: 5.7e-4, 5.3e-4 (fp16 weights), 8.8e-4, 7.3e-4 (fp32 weights); 8x = 7e-3, 6e-3: the ceiling
ENC_MOMENTS_BOUND = (2e-5, 1e-5)   # 1.26e-6, 9.6e-7 / 1.21e-6, 9.2e-7 (fp16 weights, 128^2 / 128x256); 1.43e-6, 1.13e-6 / 1.34e-6, 1.12e-6 (fp32)
ENC_GRAD_BOUND = (3e-5, 3e-5)      # cotangent O(1): 2.07e-6, 2.05e-6 ... 2.71e-6, 2.51e-6; cotangent 1e-5: 2.41e-6, 2.04e-6 ... 2.75e-6, 2.52e-6


def _watch(net, seen):
    """Forward pre-hooks that record, for every layer with a hand-written path, whether its input takes it."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance import sd_nets, transformer_cm
    handles = []

    def add(mod, fn):
        handles.append(mod.register_forward_pre_hook(fn))
    for name, m in net.named_modules():
        if isinstance(m, sd_nets.ResnetBlock2D):
            def res(mod, args, name=name):
                x = args[0]
                seen[name] = ('conv3x3', tuple(x.shape[2:]), ops.conv3x3_supported(mod.conv1, x) and ops.conv3x3_supported(mod.conv2, x))
                if mod.conv_shortcut is not None:
                    seen[name + '.conv_shortcut'] = ('conv1x1', tuple(x.shape[2:]), ops.conv1x1_supported(mod.conv_shortcut, x)
                                                     or ops.conv_gemm_supported(mod.conv_shortcut, x))
            add(m, res)
        elif isinstance(m, sd_nets.Transformer2DModel):
            add(m, lambda mod, args, name=name: seen.__setitem__(name, ('transformer', tuple(args[0].shape[2:]),
                                                                        transformer_cm.supported(mod, args[0]))))
        elif isinstance(m, sd_nets.VAEAttention):
            add(m, lambda mod, args, name=name: seen.__setitem__(name, ('vae_attention', tuple(args[0].shape[2:]),
                                                                        ops.vae_attention_supported(args[0]))))
        elif isinstance(m, sd_nets.Upsample2D):
            add(m, lambda mod, args, name=name: seen.__setitem__(name, ('conv3x3', (2 * args[0].shape[2], 2 * args[0].shape[3]), ops.conv3x3_supported(
                mod.conv, args[0], hw=(2 * args[0].shape[2], 2 * args[0].shape[3])))))         # the size it convolves at
        elif isinstance(m, sd_nets.Downsample2D):
            add(m, lambda mod, args, name=name: seen.__setitem__(name, ('conv_gemm', tuple(args[0].shape[2:]),
                                                                        ops.conv_gemm_supported(mod.conv, args[0]))))
    return handles


# ---------------------------------------------------------------------------------------------------------------- UNet
class _OneAtATime:
    """Builds (variant, module on the device, fp64 twin on the host) on demand and keeps the last variant only: the UNet is
    3.4 GB in fp32 and 6.9 GB in fp64."""

    def __init__(self, factory, seed, device):
        self.factory, self.seed, self.device, self.held = factory, seed, device, None

    def __call__(self, variant):
        if self.held is None or self.held[0] != variant:
            self.held = None
            torch.cuda.empty_cache()
            mod, twin = seeded_network(self.factory, self.seed, variant == 'fp16_weights')
            self.held = (variant, mod.to(self.device), twin)
        return self.held


@pytest.fixture(scope='module')
def unets(cuda):
    from mvip_nerf_amd.guidance import sd_nets
    get = _OneAtATime(sd_nets.UNet2DConditionModel, 5, cuda)
    yield get
    get.held = None
    torch.cuda.empty_cache()


def _unet_inputs(batch, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 9, H, W, generator=g), torch.randn(batch, 77, 768, generator=g), torch.tensor(417)


def _unet_reference(twin, x, ctx, t):
    with torch.no_grad():
        return twin(x.double(), t, encoder_hidden_states=ctx.double())[0]


def test_unet_forward_64x64_every_level_hand_written(unets, cuda):
    """Case B: batch 1, 9 x 64 x 64, fp16-representable weights: the one size at which EVERY level is on the hand-written
    path, the 8 x 8 level and the mid block (64 tokens padded to 256) included; a profiled forward lists no library
    contraction kernel."""
    variant, dev, twin = unets('fp16_weights')
    x, ctx, t = _unet_inputs(1, 64, 64, 12)
    ref = _unet_reference(twin, x, ctx, t)
    xd, cd, td = x.to(cuda), ctx.to(cuda), t.to(cuda)
    seen = {}
    handles = _watch(dev, seen)
    try:
        with torch.no_grad():
            got = dev(xd, td, encoder_hidden_states=cd)[0]
    finally:
        for h in handles:
            h.remove()
    assert all(ok for _, _, ok in seen.values()), [n for n, v in seen.items() if not v[2]]
    assert {hw for _, hw, _ in seen.values()} == {(64, 64), (32, 32), (16, 16), (8, 8)}
    assert len([1 for k, _, _ in seen.values() if k == 'transformer']) == 16 and len(seen) >= 16 + 22 + 6
    with torch.no_grad():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            again = dev(xd, td, encoder_hidden_states=cd)[0]
            torch.cuda.synchronize()
    assert torch.equal(got, again)
    names = [ev.key for ev in prof.key_averages()]
    assert not library_kernels_in(names), library_kernels_in(names)
    for must in ('conv3x3_f16x3_kernel', 'attn_f16x3'):
        assert any(must in n for n in names), must
    e = errors(got, ref)
    print(f'unet B {variant}: max {e[0]:.3e} L2 {e[1]:.3e} of eps')
    assert e[0] < UNET_BOUND[0] and e[1] < UNET_BOUND[1], e


@pytest.mark.parametrize('variant', ['fp16_weights', 'fp32_weights'])
def test_unet_forward_32x32_levels_and_library_hand_offs(unets, cuda, variant):
    """Case A: batch 2, 9 x 32 x 32, prompt 77 x 768, t = 417.  The 32^2, 16^2 and 8^2 levels run the hand-written
    3 x 3 convolutions and transformer; at the 4^2 level and in the mid block the 3 x 3 kernel and the transformer path decline
    (GroupNorm kernels + im2col GEMM convolutions; the module's own transformer: library linears and attention, its two 1 x 1
    projections on the GEMM convolution, because the library's 1 x 1 convolution at 16 pixels is not repeatable call to call): the hand-offs between the
    kinds of path are part of what is compared.  Both weight variants; then the same forward in the single-product arithmetic
    (mfma_prec = 1), which must lie ABOVE the split-precision bound and below an fp16-grade one."""
    from mvip_nerf_amd import ops
    _, dev, twin = unets(variant)
    x, ctx, t = _unet_inputs(2, 32, 32, 11)
    ref = _unet_reference(twin, x, ctx, t)
    xd, cd, td = x.to(cuda), ctx.to(cuda), t.to(cuda)
    seen = {}
    handles = _watch(dev, seen)
    try:
        with torch.no_grad():
            got = dev(xd, td, encoder_hidden_states=cd)[0]
    finally:
        for h in handles:
            h.remove()
    for name, (kind, hw, ok) in seen.items():                       # 3 x 3 convolutions and transformers: 32^2, 16^2, 8^2 hand-written,
        assert ok == (min(hw) >= 8 or kind in ('conv1x1', 'conv_gemm')), (name, kind, hw, ok)    # 4^2 not; the GEMM convolutions at any size
    assert {hw for _, hw, _ in seen.values()} >= {(32, 32), (16, 16), (8, 8), (4, 4)}
    packed = ops._conv_packed(dev.down_blocks[0].resnets[0].conv1, False)
    assert ops._prec_w(packed) == (2 if variant == 'fp16_weights' else 0)
    with torch.no_grad():
        again = dev(xd, td, encoder_hidden_states=cd)[0]            # cached prompt projections, cached _tcat, the registries
    e = errors(got, ref)
    print(f'unet A {variant}: max {e[0]:.3e} L2 {e[1]:.3e} of eps; a repeated call differs by {float((got - again).abs().max()):.3e}')
    dev.mfma_prec = 1
    try:
        with torch.no_grad():
            got16 = dev(xd, td, encoder_hidden_states=cd)[0]
    finally:
        dev.mfma_prec = 0
    with torch.no_grad():
        third = dev(xd, td, encoder_hidden_states=cd)[0]            # nothing of the other arithmetic is left in a cache
    e16 = errors(got16, ref)
    print(f'unet A {variant} single product: max {e16[0]:.3e} L2 {e16[1]:.3e} of eps')
    assert torch.equal(got, again) and torch.equal(got, third)
    assert e[0] < UNET_BOUND[0] and e[1] < UNET_BOUND[1], e
    assert UNET_BOUND[0] < e16[0] < UNET_FP16_BOUND[0] and UNET_BOUND[1] < e16[1] < UNET_FP16_BOUND[1], e16


# ---------------------------------------------------------------------------------------------------------- VAE encoder
@pytest.fixture(scope='module')
def vaes(cuda):
    from mvip_nerf_amd.guidance import sd_nets
    get = _OneAtATime(sd_nets.AutoencoderKL, 7, cuda)
    yield get
    get.held = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', [(2, 3, 128, 128), (1, 3, 128, 256)])
@pytest.mark.parametrize('variant', ['fp16_weights', 'fp32_weights'])
def test_vae_encoder_forward_and_image_gradient(vaes, cuda, variant, shape):
    """AutoencoderKL.encode: latent_dist.moments, and the gradient of scaled_sample(noise, 0.18215) under a fixed cotangent
    with respect to the input image (GroupNorm backward / ShortcutLink / absmax_scale_from_maxima chain, the VAE attention
    backward, the stride-2 and 1 x 1 convolutions on the GEMM), at cotangents of O(1) and of 1e-5 (the gradient scales are
    measured powers of two: the same relative error at both; a fixed or stale scale would show as a difference).  Levels
    128 x 128 ... 16 x 16 and the non-square 128 x 256 ... 16 x 32: every one on the hand-written path (asserted); a second
    forward + backward on the same module repeats the first bit for bit (registries, packed-weight caches)."""
    from mvip_nerf_amd import ops
    _, dev, twin = vaes(variant)
    g = torch.Generator().manual_seed(shape[3])
    x = torch.rand(shape, generator=g) * 2 - 1
    noise = torch.randn(shape[0], 4, shape[2] // 8, shape[3] // 8, generator=g)
    cot = torch.randn(noise.shape, generator=g)
    cots = (cot, cot * 1e-5)
    # fp64 on the host: one forward, one backward per cotangent
    x64 = x.double().requires_grad_(True)
    d64 = twin.encode(x64).latent_dist
    z64 = d64.scaled_sample(noise.double(), 0.18215)
    refs = [torch.autograd.grad(z64, x64, c.double(), retain_graph=True)[0] for c in cots]
    ref_m = d64.moments.detach()

    def run(c, seen=None):
        xd = x.to(cuda).requires_grad_(True)
        handles = _watch(dev, seen) if seen is not None else []
        try:
            d = dev.encode(xd).latent_dist
        finally:
            for h in handles:
                h.remove()
        d.scaled_sample(noise.to(cuda), 0.18215).backward(c.to(cuda))
        return d.moments.detach(), xd.grad
    seen = {}
    m1, g1 = run(cots[0], seen)
    assert len(seen) >= 8 + 1 + 3 + 2 and all(ok for _, _, ok in seen.values()), [n for n, v in seen.items() if not v[2]]
    assert {hw for _, hw, _ in seen.values()} == {(shape[2] >> k, shape[3] >> k) for k in range(4)}
    assert seen['encoder.mid_block.attentions.0'][0] == 'vae_attention'
    if variant == 'fp16_weights':
        assert ops._prec_w(ops._conv_packed(dev.encoder.down_blocks[0].resnets[0].conv1, False)) == 2
    else:
        assert ops._prec_w(ops._conv_packed(dev.encoder.down_blocks[0].resnets[0].conv1, False)) == 0
    m1b, g1b = run(cots[0])
    assert torch.equal(m1, m1b) and torch.equal(g1, g1b)
    m2, g2 = run(cots[1])
    assert torch.equal(m1, m2)
    em = errors(m1, ref_m)
    eg = [errors(g1, refs[0]), errors(g2, refs[1])]
    print(f'encoder {shape} {variant}: moments max {em[0]:.3e} L2 {em[1]:.3e}; image gradient, cotangent O(1): max {eg[0][0]:.3e} '
          f'L2 {eg[0][1]:.3e}; cotangent 1e-5: max {eg[1][0]:.3e} L2 {eg[1][1]:.3e}')
    assert em[0] < ENC_MOMENTS_BOUND[0] and em[1] < ENC_MOMENTS_BOUND[1], em
    for e in eg:
        assert e[0] < ENC_GRAD_BOUND[0] and e[1] < ENC_GRAD_BOUND[1], eg
