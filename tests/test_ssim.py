"""SSIM on the GPU (csrc/ssim.hip, ops.ssim) against the restatement tests/ssim_numpy.py.

The yardstick is the restatement in fp64 on the fp32 inputs.  Map: per pixel |gpu - r64| <= 2^-20 M_p, M_p the magnitude of the
terms that cancel in that pixel (ssim_numpy.magnitude_map); the fp32 restatement stays within 1.03 x 2^-22 M_p on every case
below (printed per case), the factor 4 on top is the allowance tests/test_warp.py gives a different operation order.  The
per-image mean is held to the mean of the per-pixel bounds over the counted pixels.  Gradient, with a random upstream gradient per
image: |gpu - g64| <= 4 e32 + 2^-22 max_q F_q, e32 the fp32 restatement's distance to the fp64 one on that case (the larger of the
rows-first and columns-first orders) and F_q the gradient expression with every term replaced by its absolute value; the floor
is there because e32 is exactly 0 on the constant cases while a differently ordered kernel need not be.  Every test prints its
figures.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_numpy as R                                   # noqa: E402

from mvip_nerf_amd import ops                            # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene1_small.npz')
TY, TX = ops.SSIM_TILE
_YARD, _CASES = {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def noise(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


def smooth(H, W, C, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([0.5 + 0.3 * np.sin(xx / (7.0 + c) + rs.rand() * 6) * np.cos(yy / (5.0 + 2 * c) + rs.rand() * 6) for c in range(C)], -1)
    return img[None].astype(np.float32)


def fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    return z['images'].astype(np.float32) / np.float32(255.), z['depths'].astype(np.float32) / np.float32(255.)


def make_case(name):
    """(x, y) of a named case, [N, H, W, C] fp32."""
    several = (10 + 2 * TY + 3, 10 + 2 * TX + 5)          # the map spans three tiles with a remainder, both ways
    if name == 'one_map_pixel':
        return noise((1, 11, 11, 1), 1), noise((1, 11, 11, 1), 2)
    if name == 'smallest_rgb':
        return noise((1, 11, 12, 3), 3), noise((1, 11, 12, 3), 4)
    if name == 'tile_remainders_batch2':
        return noise((2, 27, 38, 3), 5), noise((2, 27, 38, 3), 6)
    if name == 'several_tiles':
        return noise((1,) + several + (3,), 7), noise((1,) + several + (3,), 8)
    if name == 'one_channel':
        return noise((1, 20, 47, 1), 9), noise((1, 20, 47, 1), 10)
    if name == 'two_channels':
        return noise((1, 20, 47, 2), 11), noise((1, 20, 47, 2), 12)
    if name == 'four_channels':
        return noise((1, 20, 47, 4), 13), noise((1, 20, 47, 4), 14)
    if name == 'uniform_noise':
        return noise((1, 30, 41, 3), 15), noise((1, 30, 41, 3), 16)
    if name == 'smooth_plus_noise':
        s = smooth(45, 53, 3, 17)
        return np.clip(s + np.float32(0.05) * (noise(s.shape, 18) - np.float32(0.5)) * 2, 0, 1).astype(np.float32), s
    if name == 'identical':
        x = noise((1, 24, 45, 3), 19)
        return x, x.copy()
    if name == 'equal_constants':
        return np.full((1, 13, 47, 3), 0.7, np.float32), np.full((1, 13, 47, 3), 0.7, np.float32)
    if name == 'different_constants':
        return np.full((1, 13, 47, 3), 0.7, np.float32), np.full((1, 13, 47, 3), 0.2, np.float32)
    if name == 'all_zeros':
        return np.zeros((1, 13, 47, 3), np.float32), np.zeros((1, 13, 47, 3), np.float32)
    if name == 'fixture_rgb':
        img, _ = fixture()
        return np.ascontiguousarray(img[:2, :, 1:]), np.ascontiguousarray(img[:2, :, :-1])
    if name == 'fixture_depth':
        _, d = fixture()
        return np.ascontiguousarray(d[0:1, :, :, None]), np.ascontiguousarray(d[1:2, :, :, None])
    raise KeyError(name)


CASES = ['one_map_pixel', 'smallest_rgb', 'tile_remainders_batch2', 'several_tiles', 'one_channel', 'two_channels', 'four_channels',
         'uniform_noise', 'smooth_plus_noise', 'identical', 'equal_constants', 'different_constants', 'all_zeros', 'fixture_rgb',
         'fixture_depth']
NOISE_CASES = ('one_map_pixel', 'smallest_rgb', 'tile_remainders_batch2', 'several_tiles', 'one_channel', 'two_channels',
               'four_channels', 'uniform_noise')


def case(name):
    if name not in _CASES:
        x, y = make_case(name)
        gout = np.random.RandomState(len(name) + 100).uniform(0.5, 1.5, x.shape[0]).astype(np.float32) \
            * np.where(np.arange(x.shape[0]) % 2 == 0, 1, -1).astype(np.float32)
        _CASES[name] = (x, y, gout)
    return _CASES[name]


def yardstick(name, mask=None, key=None):
    """The restatement's figures of a case, computed once and left unchanged."""
    key = (name, key)
    if key not in _YARD:
        x, y, gout = case(name)
        _YARD[key] = R.yardstick(x, y, gout, mask)
    return _YARD[key]


def gpu_ssim(cuda, x, y, gout=None, mask=None):
    """(ssim [N], map, count [N], grad [N, H, W, C] or None) as numpy."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(cuda).requires_grad_(gout is not None)
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(cuda)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(cuda)
    s, smap, count = ops.ssim(xt, yt, mask=mt, return_map=True, return_count=True)
    assert s.dtype == torch.float32 and smap.dtype == torch.float32 and count.dtype == torch.int32
    assert tuple(s.shape) == (x.shape[0],) and tuple(smap.shape) == (x.shape[0], x.shape[1] - 10, x.shape[2] - 10, x.shape[3])
    assert not smap.requires_grad and s.requires_grad == (gout is not None)
    grad = None
    if gout is not None:
        (s * torch.from_numpy(gout).to(cuda)).sum().backward()
        grad = xt.grad.cpu().numpy()
    return s.detach().cpu().numpy(), smap.cpu().numpy(), count.cpu().numpy(), grad


def check(name, cuda, mask=None, key=None):
    x, y, gout = case(name)
    yd = yardstick(name, mask, key)
    s, smap, count, grad = gpu_ssim(cuda, x, y, gout, mask)
    C = x.shape[-1]
    assert np.array_equal(count, yd['count'])
    assert np.isfinite(smap).all() and np.isfinite(s).all() and np.isfinite(grad).all()
    # the map
    bound = 2.0 ** -20 * yd['M']
    err = np.abs(smap.astype(np.float64) - yd['map'])
    r32 = float((yd['map32_err'] / yd['M']).max() * 2.0 ** 22)
    print(f'{name}: ssim {s.tolist()} (fp64 {yd["ssim"].tolist()}), count {count.tolist()}; map error up to {err.max():.3e} = '
          f'{float((err / yd["M"]).max()) * 2 ** 22:.2f} x 2^-22 M (fp32 restatement {r32:.2f}), M up to {yd["M"].max():.1f}')
    assert r32 <= 1.03
    assert (err <= bound).all()
    # the mean: within the mean of the per-pixel bounds over what is counted
    w = R.counted(x.shape, mask)[..., None] * np.ones(C)
    mean_bound = np.where(count > 0, (bound * w).reshape(len(count), -1).sum(1) / np.maximum(count * C, 1), 0.0)
    mean_err = np.abs(s.astype(np.float64) - yd['ssim'])
    print(f'{name}: mean error {mean_err.tolist()}, bound {mean_bound.tolist()}')
    assert (mean_err <= mean_bound).all()
    assert (s[count == 0] == 1.0).all()
    # the gradient
    g_err = float(np.abs(grad.astype(np.float64) - yd['grad']).max())
    g_bound = 4.0 * yd['e32'] + 2.0 ** -22 * float(yd['F'].max())
    g_max = float(np.abs(yd['grad']).max())
    print(f'{name}: gradient up to {g_max:.3e}, error {g_err:.3e}, e32 {yd["e32"]:.3e}, max F {yd["F"].max():.3e}, bound {g_bound:.3e}'
          + (f' = {g_bound / g_max:.2e} of the largest entry' if g_max > 0 else ''))
    assert g_err <= g_bound
    return s, smap, count, grad


@pytest.mark.parametrize('name', CASES)
def test_case_meets_the_bounds(name, cuda):
    x, y, _ = case(name)
    s, smap, count, grad = check(name, cuda)
    assert (count == (x.shape[1] - 10) * (x.shape[2] - 10)).all()
    yd = yardstick(name)
    if name in NOISE_CASES:
        # a wrong tap or halo cannot hide under the bound: the smallest tap is 1.0e-3 of the window, the bound 1e-5 of the
        # largest gradient entry (2.4e-6 to 4.5e-6 on these cases)
        assert 4.0 * yd['e32'] + 2.0 ** -22 * float(yd['F'].max()) <= 1e-5 * float(np.abs(yd['grad']).max())
    # closed forms, to the map bound plus the window's sum (1 only to the rounding of its fp32 taps: 2e-6, tests/test_ssim_cpu.py)
    closed = 2.0 ** -20 * float(yd['M'].max()) + 2e-6
    if name in ('identical', 'equal_constants', 'all_zeros'):
        assert np.abs(s - 1.0).max() <= closed
    if name == 'different_constants':
        a, b = float(np.float32(0.7)), float(np.float32(0.2))
        assert abs(float(s[0]) - (2 * a * b + R.C1) / (a * a + b * b + R.C1)) <= closed
    if name == 'several_tiles':
        assert -(-smap.shape[1] // TY) >= 3 and smap.shape[1] % TY and -(-smap.shape[2] // TX) >= 3 and smap.shape[2] % TX


# ---- masks ----------------------------------------------------------------------------------------------------------------------

def test_random_mask(cuda):
    x, _, _ = case('tile_remainders_batch2')
    mask = np.random.RandomState(30).rand(*x.shape[:3]) < 0.4
    _, _, count, _ = check('tile_remainders_batch2', cuda, mask, 'random')
    assert (count > 0).all() and (count < 17 * 28).all()


def test_mask_that_touches_the_borders(cuda):
    x, y, gout = case('several_tiles')
    H, W = x.shape[1:3]
    mask = np.zeros((1, H, W), bool)
    mask[:, H // 2 - 2:H // 2 + 3, :] = True                 # a cross through the centre out to all four borders
    mask[:, :, W // 2 - 2:W // 2 + 3] = True
    _, _, count, grad = check('several_tiles', cuda, mask, 'cross')
    assert count[0] == 5 * (W - 10) + 5 * (H - 10) - 25      # the border band of 5 is not counted
    band = np.ones((1, H, W), bool)
    band[:, 5:H - 5, 5:W - 5] = False                        # the border band alone: no map pixel at all
    s, _, count, grad = check('several_tiles', cuda, band, 'band')
    assert count[0] == 0 and s[0] == 1.0 and not bits(grad).any()


def test_one_empty_mask_in_a_batch(cuda):
    x, y, gout = case('tile_remainders_batch2')
    mask = np.zeros(x.shape[:3], bool)
    mask[1, 4:20, 7:30] = True
    s, smap, count, grad = check('tile_remainders_batch2', cuda, mask, 'one_empty')
    assert count.tolist() == [0, 15 * 23] and s[0] == 1.0 and not bits(grad[0]).any() and grad[1].any()
    solo = gpu_ssim(cuda, x[1:], y[1:], gout[1:], mask[1:])
    assert np.array_equal(bits(s[1:]), bits(solo[0])) and np.array_equal(bits(smap[1]), bits(solo[1][0]))
    assert np.array_equal(bits(grad[1]), bits(solo[3][0]))


# ---- reproducibility and interface ---------------------------------------------------------------------------------------------------

def test_repetition_and_batch_are_bit_equal(cuda):
    rs = np.random.RandomState(40)
    H, W = 10 + TY + 7, 10 + 2 * TX + 9
    x, y = rs.rand(3, H, W, 3).astype(np.float32), rs.rand(3, H, W, 3).astype(np.float32)
    gout = np.array([1.0, -0.5, 2.0], np.float32)
    mask = rs.rand(3, H, W) < 0.7
    for m in (None, mask):
        a = gpu_ssim(cuda, x, y, gout, m)
        b = gpu_ssim(cuda, x, y, gout, m)
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
        for k in range(3):
            one = gpu_ssim(cuda, x[k:k + 1], y[k:k + 1], gout[k:k + 1], None if m is None else m[k:k + 1])
            assert all(np.array_equal(bits(p[0]), bits(q[k])) for p, q in zip(one, a)), k
        # the mean does not depend on whether the map or the gradient is asked for
        xt, yt = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda)
        mt = None if m is None else torch.from_numpy(m).to(cuda)
        plain = ops.ssim(xt, yt, mask=mt)
        assert torch.is_tensor(plain) and np.array_equal(bits(plain.cpu().numpy()), bits(a[0]))


def test_interface(cuda):
    x = torch.rand((2, 14, 15, 3), device=cuda)
    y = torch.rand((2, 14, 15, 3), device=cuda)
    s = ops.ssim(x, y)
    assert s.grad_fn is None and not s.requires_grad and tuple(s.shape) == (2,)      # no-grad input: no grad_fn
    s, smap = ops.ssim(x, y, return_map=True)
    assert smap.grad_fn is None and tuple(smap.shape) == (2, 4, 5, 3)
    yg = y.clone().requires_grad_(True)
    assert ops.ssim(x, yg).grad_fn is None                                            # y is detached
    xg = x.clone().requires_grad_(True)
    s = ops.ssim(xg, y)
    assert s.grad_fn is not None
    (1.0 - s).mean().backward()
    assert xg.grad is not None and tuple(xg.grad.shape) == tuple(x.shape) and xg.grad.abs().max() > 0
    with torch.no_grad():
        assert ops.ssim(xg, y).grad_fn is None
    # N = 0: empty tensors, nothing launched
    e = ops.ssim(x[:0], y[:0])
    assert tuple(e.shape) == (0,) and e.dtype == torch.float32
    e, emap = ops.ssim(x[:0], y[:0], return_map=True)
    assert tuple(emap.shape) == (0, 4, 5, 3)
    with pytest.raises(ValueError, match='contiguous'):
        ops.ssim(x.transpose(1, 2), y.transpose(1, 2))
    with pytest.raises(ValueError, match='one device|GPU'):
        ops.ssim(x, y.cpu())
