"""What tests/test_sd_networks.py and test_sds.py::test_epilogue_moments_under_a_large_group_mean rest on, checked without a GPU
(tests/sd_network_cases.py): the seeded weights and their fp64 twin, the error metrics, the large-mean inputs, and a numpy
restatement of the two summation orders of the unsplit convolution's epilogue moments (csrc/conv3x3.hip)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sd_network_cases import errors, large_mean_residual, library_kernels_in, seeded_network     # noqa: E402


def test_seeded_network_and_its_fp64_twin():
    """The twin holds exactly the module's values, fp16 rounding is exact, the norms are off 1 / 0, everything is frozen; and
    the fp32 host evaluation of a small encoder (a dozen layers at u = 6e-8 each) sits below a tenth of the 1e-4 the device
    path is held to -- the tolerance is the kernels' to spend."""
    from mvip_nerf_amd.guidance import sd_nets
    for fp16 in (True, False):
        mod, twin = seeded_network(lambda: sd_nets.Encoder(block_out=(32, 64), latent=4), 3, fp16)
        for (n, p), (n2, q) in zip(mod.named_parameters(), twin.named_parameters()):
            assert n == n2 and q.dtype == torch.float64 and not p.requires_grad and not q.requires_grad
            assert torch.equal(p.double(), q)
            assert torch.equal(p.half().float(), p) == fp16 or p.numel() < 8
        g = mod.conv_norm_out
        assert float((g.weight - 1).abs().max()) > 0.1 and float(g.bias.abs().max()) > 0.1
        x = torch.rand(1, 3, 16, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
        with torch.no_grad():
            e = errors(mod(x), twin(x.double()))
        assert e[0] < 1e-5 and e[1] < 1e-5, e
    a, b = seeded_network(lambda: sd_nets.Encoder(block_out=(32, 64)), 3, True)[0], seeded_network(lambda: sd_nets.Encoder(block_out=(32, 64)), 3, True)[0]
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))           # seeded: the same weights every time


def test_error_metrics_and_banned_names():
    ref = torch.tensor([3.0, -4.0], dtype=torch.float64)
    e = errors(torch.tensor([3.0, -4.5]), ref)
    assert abs(e[0] - 0.125) < 1e-12 and abs(e[1] - 0.1) < 1e-12
    names = ['void mvip::conv3x3_f16x3_kernel<2, 32, 4, 2>(mvip::ConvArgs)', 'Cijk_Ailk_Bljk_SB_MT64x64', 'mvip::attn_f16x3_kernel',
             'void at::native::(anonymous namespace)::softmax_warp_forward<float>', 'attn_fwd', 'mvip::gemm_f16x3_kernel<1>']
    assert library_kernels_in(names) == [names[1], names[3], names[4]]


def test_large_mean_residual_ratios():
    for ratio in (10, 30, 100):
        for per_channel in (False, True):
            r = large_mean_residual((2, 128, 8, 32), ratio, per_channel, torch.Generator().manual_seed(ratio)).double()
            rg = r.reshape(2, 32, -1)
            got = float((rg.mean(-1) / rg.std(-1)).median())
            assert (0.45 if per_channel else 0.9) * ratio < got < 1.1 * ratio, (ratio, per_channel, got)
            rows = r.mean((2, 3))                # channel means: sampling noise 0.5 / sqrt(256) = 0.031 alone, or the offsets' spread as well
            assert (float(rows.std()) > 1.5 * 0.5 / 16) == per_channel, (ratio, per_channel, float(rows.std()))


def _tree64(v):
    """fp32 sum of the last axis (64 values) as a balanced tree: the depth and rounding count of the epilogue's DPP steps."""
    v = v.astype(np.float32)
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _rstd_error(y, shifted):
    w = y.reshape(-1, 64)
    if shifted:                                  # per 64 values: sums about K = the first of them; raw moments restored in fp64
        k32 = w[:, :1]
        d = (w - k32).astype(np.float32)
        s, q = _tree64(d).astype(np.float64), _tree64((d * d).astype(np.float32)).astype(np.float64)
        k = k32[:, 0].astype(np.float64)
        S, Q = (s + 64.0 * k).sum(), (q + k * (2.0 * s + 64.0 * k)).sum()
    else:                                        # raw fp32 squares
        S, Q = _tree64(w).astype(np.float64).sum(), _tree64((w * w).astype(np.float32)).astype(np.float64).sum()
    mean = S / y.size
    ref = 1.0 / np.sqrt(y.astype(np.float64).var() + 1e-5)
    return abs(1.0 / np.sqrt(Q / y.size - mean * mean + 1e-5) - ref) / ref


def test_moment_partials_about_a_shift_restatement():
    """E[y^2] - mean^2 from fp32 partials of 64 values, fp64 afterwards, for groups of 2,048 values at mean / std = 100.
    About a shift K taken from the 64 values themselves every term of a partial is (y - K)^2 >= 0 with E (y - K)^2 = 2 var: a
    tree of depth 6 over rounded squares errs by at most 7 u of the partial, so the variance by 14 u and rstd by 7 u = 4.2e-7
    (u = 2^-24), whatever the mean.  The raw squares err by the same 7 u of sum y^2 = (1 + ratio^2) n var: the bound grows with
    ratio^2, and the observed median at ratio 100 is above 1e-5 -- three times the 3e-6 floor the consumer is held to."""
    rs = np.random.RandomState(0)
    u = 2.0 ** -24
    for ratio, raw_floor in ((10, 0.0), (100, 1e-5)):
        raw, shifted = [], []
        for _ in range(50):
            y = (rs.randn(2048) * 0.5 + 0.5 * ratio).astype(np.float32)
            raw.append(_rstd_error(y, False))
            shifted.append(_rstd_error(y, True))
        assert max(shifted) <= 7 * u, (ratio, max(shifted))
        assert np.median(raw) >= raw_floor and max(raw) <= 7 * u * (1 + ratio ** 2), (ratio, np.median(raw), max(raw))
