"""SSIM without a GPU: the restatement (tests/ssim_numpy.py) against a fp64 torch conv2d composition and its autograd, the
closed forms (x = y, constants, symmetry), the figures of the conditioning note on the scene fixture, the argument checks of the
C entry points with NULL operands, ops.ssim's refusals, and the host-only helpers of mvip_nerf_amd/evaluate.py."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_numpy as R                                   # noqa: E402

from mvip_nerf_amd import _lib, evaluate, ops            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
OK, EINVAL = 0, -1
P0 = None            # NULL


def torch_ssim(x, y, mask=None):
    """SSIM as a torch composition in fp64, written from the formula and not from ssim_numpy: one grouped conv2d with the 2D
    window on the five products, then elementwise ops.  x, y [N, H, W, C] fp64 tensors.  Returns (ssim [N], map [N, H-10, W-10, C])."""
    N, H, W, C = x.shape
    g = torch.from_numpy(R.window(np.float64))
    k2 = torch.outer(g, g)[None, None].repeat(5 * C, 1, 1, 1)
    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    m = F.conv2d(torch.cat([xc, yc, xc * xc, yc * yc, xc * yc], 1), k2, groups=5 * C)
    mx, my, exx, eyy, exy = m.split(C, 1)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = ((2 * mx * my + R.C1) * (2 * sxy + R.C2)) / ((mx * mx + my * my + R.C1) * (sxx + syy + R.C2))
    s = s.permute(0, 2, 3, 1)
    w = torch.ones((N, H - 10, W - 10), dtype=torch.float64) if mask is None else torch.from_numpy(mask[:, 5:H - 5, 5:W - 5].astype(np.float64))
    cnt = w.sum((1, 2))
    mean = torch.where(cnt > 0, (s * w[..., None]).sum((1, 2, 3)) / (cnt.clamp(min=1) * C), torch.ones_like(cnt))
    return mean, s


def noise_pair(N, H, W, C, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(N, H, W, C).astype(np.float32), rs.rand(N, H, W, C).astype(np.float32)


def test_window():
    g = R.window()
    assert g.shape == (11,) and np.array_equal(g, g[::-1]) and abs(g.sum() - 1.0) < 1e-7
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g)      # fp32 values
    e = np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5)
    assert np.abs(g - e / e.sum()).max() < 2.0 ** -25


def test_restatement_equals_the_torch_composition():
    for (N, H, W, C), seed in (((2, 17, 23, 3), 0), ((1, 11, 11, 1), 1), ((2, 13, 30, 4), 2)):
        x, y = noise_pair(N, H, W, C, seed)
        mask = np.random.RandomState(seed + 10).rand(N, H, W) < 0.5
        for m in (None, mask):
            want, want_map = torch_ssim(torch.from_numpy(x).double(), torch.from_numpy(y).double(), m)
            got, got_map, count = R.ssim(x, y, m)
            assert got_map.shape == (N, H - 10, W - 10, C)
            assert np.abs(got_map - want_map.numpy()).max() <= 1e-12 and np.abs(got - want.numpy()).max() <= 1e-12
            assert np.array_equal(count, (m[:, 5:-5, 5:-5].sum((1, 2)) if m is not None else np.full(N, (H - 10) * (W - 10))))


def test_closed_form_gradient_equals_autograd():
    for (N, H, W, C), seed in (((2, 17, 23, 3), 3), ((1, 12, 11, 1), 4)):
        x, y = noise_pair(N, H, W, C, seed)
        rs = np.random.RandomState(seed + 20)
        gout = rs.randn(N).astype(np.float32)
        mask = rs.rand(N, H, W) < 0.6
        for m in (None, mask):
            xt = torch.from_numpy(x).double().requires_grad_(True)
            mean, _ = torch_ssim(xt, torch.from_numpy(y).double(), m)
            (mean * torch.from_numpy(gout).double()).sum().backward()
            want = xt.grad.numpy()
            got = R.grad(x, y, gout, m)
            rel = np.abs(got - want).max() / np.abs(want).max()
            print(f'gradient {N}x{H}x{W}x{C} mask {m is not None}: max {np.abs(want).max():.3e}, relative difference {rel:.2e}')
            assert rel <= 1e-12
            # the magnitude plane bounds the gradient it is the magnitude of
            assert (R.magnitude_grad(x, y, gout, m) >= np.abs(got) * (1 - 1e-12)).all()


def test_identities():
    x, y = noise_pair(2, 19, 16, 3, 5)
    s, smap, _ = R.ssim(x, x)
    assert np.abs(smap - 1.0).max() <= 1e-12 and np.abs(s - 1.0).max() <= 1e-12      # x = y gives 1
    a, b = 0.7, 0.2
    ca, cb = np.full((1, 13, 14, 2), a, np.float32), np.full((1, 13, 14, 2), b, np.float32)
    a32, b32 = float(np.float32(a)), float(np.float32(b))
    want = (2 * a32 * b32 + R.C1) / (a32 * a32 + b32 * b32 + R.C1)
    # constants: the luminance factor alone -- up to the window's sum, which is 1 only to the rounding of its fp32 taps:
    # E[xy] - mu_x mu_y = a b S (1 - S) for S = sum g, and likewise in the denominator, against C2
    tol = 2.0 * (a + b) ** 2 * abs(1.0 - R.window().sum()) / R.C2
    assert 0 < tol < 1e-5
    assert np.abs(R.ssim(ca, cb)[1] - want).max() <= tol
    assert np.abs(R.ssim(ca, ca)[1] - 1.0).max() <= tol
    assert np.abs(R.ssim(x, y)[1] - R.ssim(y, x)[1]).max() <= 1e-14                   # symmetric in x, y
    assert np.abs(R.ssim(np.zeros_like(x), np.zeros_like(x))[1] - 1.0).max() == 0.0   # black against black
    # an empty mask: exactly 1, a zero gradient, and no trace in the other image
    mask = np.zeros((2, 19, 16), bool)
    mask[1, 5:9, 5:8] = True
    s, _, count = R.ssim(x, y, mask)
    g = R.grad(x, y, np.ones(2, np.float32), mask)
    assert s[0] == 1.0 and count.tolist() == [0, 12] and not g[0].any() and g[1].any()
    assert np.array_equal(g[1], R.grad(x[1:], y[1:], np.ones(1, np.float32), mask[1:])[0])
    # the border band of a mask has no map pixel
    band = np.ones((2, 19, 16), bool)
    band[:, 5:-5, 5:-5] = False
    assert R.ssim(x, y, band)[2].tolist() == [0, 0]


def test_fp32_restatement_on_the_fixture():
    """The conditioning note of DESIGN.md section 16: on 8-bit images the raw-moment form loses digits per map pixel (sigma^2
    cancels against brightness^2 over C2), the per-image mean does not; and the fp32 run stays inside the map bound's unit."""
    z = np.load(FIXTURE, allow_pickle=False)
    img = z['images'][:2].astype(np.float32) / np.float32(255.)
    x, y = np.ascontiguousarray(img[:, :, 1:]), np.ascontiguousarray(img[:, :, :-1])
    s64, m64, _ = R.ssim(x, y)
    s32, m32, _ = R.ssim(x, y, dtype=np.float32)
    err = np.abs(m32.astype(np.float64) - m64)
    M = R.magnitude_map(x, y)
    print(f'fixture: ssim {s64}, per-pixel fp32 error up to {err.max():.2e} ({(err / M).max() * 2 ** 22:.2f} x 2^-22 M), mean off by '
          f'{np.abs(s32.astype(np.float64) - s64).max():.2e}, M up to {M.max():.0f}')
    assert 1e-5 <= err.max() <= 1e-3
    assert (err <= 2.0 ** -20 * M).all()
    assert np.abs(s32.astype(np.float64) - s64).max() <= 1e-6


def test_entry_point_argument_checks():
    sig = _lib._SIGNATURES
    assert _lib.ABI_VERSION == 5
    assert all(n in _lib.DECLARED_SYMBOLS for n in ('mvip_ssim_tiles', 'mvip_ssim_forward', 'mvip_ssim_backward'))
    assert len(sig['mvip_ssim_forward'][1]) == 14 and len(sig['mvip_ssim_backward'][1]) == 11
    lib = _lib.load()
    fwd = lambda N, H, W, C: lib.mvip_ssim_forward(P0, P0, P0, N, H, W, C, P0, P0, P0, P0, P0, P0, P0)
    bwd = lambda N, H, W, C: lib.mvip_ssim_backward(P0, P0, P0, P0, P0, N, H, W, C, P0, P0)
    for call in (fwd, bwd):
        for N, H, W, C in ((-1, 20, 20, 3), (2, 10, 20, 3), (2, 20, 10, 3), (2, 0, 0, 3), (2, 20, 20, 0), (2, 20, 20, 5), (2, 20, 20, -1),
                           (2, 16385, 20, 3), (2, 20, 16385, 3), (1 << 31, 20, 20, 3), (0, 10, 20, 3), (0, 20, 20, 5)):
            assert call(N, H, W, C) == EINVAL, (N, H, W, C)
        assert call(0, 11, 11, 1) == OK and call(0, 20, 20, 4) == OK            # no image: nothing launched
        assert call(2, 20, 20, 3) == EINVAL                                     # NULL operands
    # the tile count the workspace is sized by, from the tile constants ops exports
    ty, tx = ops.SSIM_TILE
    assert (ty, tx) == (16, 32) and ops.SSIM_WINDOW == 11
    for H, W in ((11, 11), (27, 38), (141, 252), (1134, 2016), (16384, 16384)):
        assert lib.mvip_ssim_tiles(H, W) == -(-(H - 10) // ty) * -(-(W - 10) // tx), (H, W)
    assert lib.mvip_ssim_tiles(10, 20) == -1 and lib.mvip_ssim_tiles(20, 16385) == -1


def test_ops_ssim_refuses_bad_arguments():
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    good = lambda: dict(x=z(2, 12, 13, 3), y=z(2, 12, 13, 3))

    def check(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.ssim(**dict(good(), **kw))
    check('GPU')                                                          # CPU tensors: no CPU fallback
    check('no CPU fallback')
    check('GPU', x=np.zeros((2, 12, 13, 3), np.float32))
    check('float32', x=z(2, 12, 13, 3, dtype=torch.float64))
    check('float32', y=z(2, 12, 13, 3, dtype=torch.float16))
    check(r'\[N, H, W, C\]', x=z(12, 13, 3))
    check('one shape', y=z(2, 12, 14, 3))
    check('channels', x=z(2, 12, 13, 5), y=z(2, 12, 13, 5))
    check('11 x 11', x=z(2, 10, 13, 3), y=z(2, 10, 13, 3))
    check('11 x 11', x=z(2, 12, 9, 3), y=z(2, 12, 9, 3))
    check('mask', mask=z(2, 12, 13, dtype=torch.uint8))
    check('mask', mask=z(2, 12, 14, dtype=torch.bool))
    check('mask', mask=np.zeros((2, 12, 13), bool))
    check('contiguous', x=z(2, 13, 12, 3).transpose(1, 2))
    check('contiguous', y=z(2, 12, 13, 4)[..., :3])
    p = inspect.signature(ops.ssim).parameters
    assert list(p)[:4] == ['x', 'y', 'mask', 'return_map'] and p['mask'].default is None and p['return_map'].default is False


def test_evaluate_host_helpers(tmp_path):
    m = np.zeros((20, 30), bool)
    assert evaluate.mask_bbox(m) is None
    m[3, 7] = m[11, 4] = m[5, 22] = True
    assert evaluate.mask_bbox(m) == (3, 12, 4, 23)
    assert evaluate.mask_bbox(torch.from_numpy(m)) == (3, 12, 4, 23)
    full = np.ones((4, 5), bool)
    assert evaluate.mask_bbox(full) == (0, 4, 0, 5)
    with pytest.raises(ValueError, match='H, W'):
        evaluate.mask_bbox(np.zeros((2, 3, 4), bool))
    # pairing: by stem, in sorted order, whatever order the lists come in
    pairs = evaluate.pair_names(['b.png', 'a.png', 'c.png'], ['c.jpg', 'a.png', 'b.png'])
    assert pairs == [('a', 'a.png', 'a.png'), ('b', 'b.png', 'b.png'), ('c', 'c.png', 'c.jpg')]
    with pytest.raises(ValueError, match='without a partner'):
        evaluate.pair_names(['a.png', 'b.png'], ['a.png'])
    with pytest.raises(ValueError, match='without a partner'):
        evaluate.pair_names(['a.png'], ['a.png', 'd.png'])
    with pytest.raises(ValueError, match='share the name'):
        evaluate.pair_names(['a.png', 'a.jpg'], ['a.png'])
    assert evaluate.pair_names([], []) == []
    assert evaluate.mean_of([1.0, None, 3.0]) == 2.0 and evaluate.mean_of([None]) is None and evaluate.mean_of([]) is None
    rep = evaluate.summarise({'psnr': [20.0, 30.0], 'ssim_bbox': [None, 0.5]})
    assert rep['views'] == 2 and rep['mean'] == {'psnr': 25.0, 'ssim_bbox': 0.5}
    path = evaluate.write_report(str(tmp_path / 'deep' / 'report.json'), rep)
    assert evaluate.read_report(path) == rep and json.load(open(path)) == rep
    # a folder with a lone name is refused before anything touches a GPU
    (tmp_path / 'p').mkdir()
    (tmp_path / 'g').mkdir()
    (tmp_path / 'p' / 'a.png').write_bytes(b'')
    with pytest.raises(ValueError, match='without a partner'):
        evaluate.evaluate_folders(str(tmp_path / 'p'), str(tmp_path / 'g'), device=torch.device('cpu'))
    assert list(inspect.signature(evaluate.image_metrics).parameters) == ['pred', 'gt', 'mask']
    assert list(inspect.signature(evaluate.evaluate_views).parameters) == ['render_kwargs', 'hwf', 'poses', 'images', 'near', 'far', 'masks',
                                                                           'disparities', 'chunk']
    assert list(inspect.signature(evaluate.evaluate_folders).parameters)[:3] == ['pred_dir', 'gt_dir', 'mask_dir']


def test_tools_help():
    for tool, opts in (('evaluate.py', ('--checkpoint', '--datadir', '--pred', '--gt', '--masks', '--out')),
                       ('ssim_bench.py', ('--repeats', '--out'))):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), '--help'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for opt in opts:
            assert opt in r.stdout, (tool, opt)
