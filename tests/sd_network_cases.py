"""What tests/test_sd_networks.py, tests/test_sd_sampler.py and tests/test_sds.py share about the SDS networks: the kernel names
that betray a library contraction in a profile, the seeded weights of the whole-network tests with their fp64 host twin, the
two error metrics, and the inputs that give a convolution's output a large per-group mean."""
import copy

import torch

# Kernel-name fragments of the library convolutions, GEMMs, attention, softmax and up-sampling (MIOpen, rocBLAS / hipBLASLt
# Tensile, CK, AOTriton, ATen): none may appear in a profile of a path that is meant to run the hand-written kernels only.
LIBRARY_CONTRACTION_KERNELS = ('igemm', 'miopen', 'naive_conv', 'Im2d2Col', 'Col2Im', 'batched_transpose', 'Cijk_', 'attn_fwd',
                               'ck::', 'grouped_conv', 'MIOpen', 'gemm_kernel', 'softmax_warp', 'SoftMax', 'upsample_nearest')


def library_kernels_in(names):
    return [n for n in names if any(b in n for b in LIBRARY_CONTRACTION_KERNELS)]


def seeded_network(factory, seed, fp16_weights):
    """(module fp32 on the host, its fp64 twin): default initialisation under `seed`, every GroupNorm / LayerNorm weight and bias
    moved away from 1 / 0 (a gamma / beta or channel mix-up must change the result), optionally every parameter rounded to an
    fp16 value (what SDNetworks ships: the packers then choose the two-product kernels), all parameters frozen.  The twin holds
    exactly the same values."""
    torch.manual_seed(seed)
    mod = factory().eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.GroupNorm, torch.nn.LayerNorm)):
                m.weight.add_(torch.randn(m.weight.shape, generator=gen) * 0.2)
                m.bias.add_(torch.randn(m.bias.shape, generator=gen) * 0.2)
        if fp16_weights:
            for p in mod.parameters():
                p.copy_(p.half().float())
    for p in mod.parameters():
        p.requires_grad_(False)
    twin = copy.deepcopy(mod).double()
    for p in twin.parameters():
        p.requires_grad_(False)
    return mod, twin


def errors(got, ref):
    """(max |got - ref| / max |ref|, |got - ref|_2 / |ref|_2) of a device tensor against its fp64 host reference."""
    g, r = got.detach().cpu().double(), ref.detach().double()
    d = g - r
    return float(d.abs().max() / r.abs().max()), float(d.norm() / r.norm())


def large_mean_residual(shape, ratio, per_channel, gen):
    """A residual [N, C, H, W] of standard deviation 0.5 around the offset 0.5 * ratio (mean / std = ratio); per_channel: every
    channel sits at a mean of its own, up to 2 % of the offset away, so that the channels of one group differ by about two
    standard deviations at ratio 100."""
    N, C, H, W = shape
    r = torch.randn(shape, generator=gen) * 0.5 + 0.5 * ratio
    if per_channel:
        r = r + (2 * torch.rand(1, C, 1, 1, generator=gen) - 1) * (0.02 * 0.5 * ratio)
    return r
