"""Inpainted-depth preparation on the GPU (mvip_nerf_amd/prepare.py, ops.harmonic_fill, ops.mask_dilate2d,
csrc/harmonic.hip) against the restatement tests/harmonic_numpy.py.

The yardstick of the fill is the fp64 direct solve of the same linear system.  Bound per case:
max |u_gpu - u_fp64| <= 4 * e32, e32 = the max error of the restatement's own fp32 conjugate-gradient run on that case against
the fp64 solve, computed here (the factor 4 covers a different summation order), and never above max |v_K| / 2550, a tenth
of the 8-bit step of the file format.  Every test prints the figures it asserts on.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harmonic_cases as C                               # noqa: E402
import harmonic_numpy as R                               # noqa: E402

import bench                                             # noqa: E402
from mvip_nerf_amd import ops, prepare, run              # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene1_small.npz')
_REF = {}


def reference(name, v=None, m=None):
    """(v, m, U, fp64 solve, e32, iterations of the fp32 restatement, bound) of a case, computed once and left unchanged."""
    if name not in _REF:
        if v is None:
            v, m = C.case(name)
        U = R.unknown_set(v, m)
        f64, singular = R.solve(v, m)
        assert not singular
        c32, it32, ok = R.cg32(v, m)
        assert ok
        e32 = float(np.abs(c32.astype(np.float64) - f64)[U].max())
        ceiling = float(np.abs(v[~U]).max()) / 2550.0
        for a in (v, m, U, f64):
            a.setflags(write=False)
        _REF[name] = (v, m, U, f64, e32, it32, min(4.0 * e32, ceiling))
    return _REF[name]


def fill(cuda, v, m, **kw):
    out, info = ops.harmonic_fill(torch.from_numpy(np.array(v)).to(cuda), torch.from_numpy(np.array(m)).to(cuda), **kw)    # copies: the cached cases are read-only
    return out.cpu().numpy(), info


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1, 2. the fill against the fp64 direct solve; structure ------------------------------------------------------------------

@pytest.mark.parametrize('name', C.ALL)
def test_fill_equals_fp64_direct_solve(name, cuda):
    v, m, U, f64, e32, it32, bound = reference(name)
    got, info = fill(cuda, v[None], m[None])
    got = got[0]
    err = float(np.abs(got.astype(np.float64) - f64)[U].max())
    print(f'{name}: unknowns {int(U.sum())}, gpu error {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}, iterations gpu '
          f'{int(info["iterations"][0])} / restatement {it32}, true residual {float(info["residual"][0]):.3e}')
    assert info['unknowns'][0] == U.sum() and info['converged'][0] and not info['singular'][0]
    if name == 'disc200':
        assert U.sum() == 125609
    assert err <= 4.0 * e32
    assert err <= float(np.abs(v[~U]).max()) / 2550.0
    # structure: known finite pixels bit for bit, the maximum principle on the filled ones
    assert np.array_equal(bits(got)[~U], bits(v)[~U])
    assert np.isfinite(got).all()
    lo, hi = float(v[~U].min()), float(v[~U].max())
    assert got[U].min() >= lo - bound and got[U].max() <= hi + bound


# ---- 3. affine exactness ------------------------------------------------------------------------------------------------------

def test_affine_images_are_reconstructed_unless_the_hole_reaches_the_border(cuda):
    a = C.affine()
    v = a.astype(np.float32)
    m = np.zeros(a.shape, bool)
    m[10:30, 12:40] = True
    _, _, U, f64, e32, _, bound = reference('affine_inner', v, m)
    got, _ = fill(cuda, v[None], m[None])
    err = float(np.abs(got[0].astype(np.float64) - a)[U].max())
    print(f'affine, inner hole: gpu error against the affine function {err:.3e}, fp64 solve {np.abs(f64 - a)[U].max():.3e}, '
          f'bound {bound:.3e}')
    assert err <= bound
    m2 = m.copy()
    m2[10:30, 0:40] = True                               # reaches the left border: the mirror boundary is not affine
    _, _, U2, f64b, _, _, bound2 = reference('affine_border', v.copy(), m2)
    assert np.abs(f64b - a)[U2].max() > 0.01
    got2, _ = fill(cuda, v[None], m2[None])
    err2 = float(np.abs(got2[0].astype(np.float64) - f64b)[U2].max())
    print(f'affine, hole on the border: gpu error against the fp64 solve {err2:.3e}, bound {bound2:.3e}, fp64 solve against '
          f'the affine function {np.abs(f64b - a)[U2].max():.3e}')
    assert err2 <= bound2


# ---- 4. batches -------------------------------------------------------------------------------------------------------------------

def test_batch_equals_single_calls_bit_for_bit(cuda):
    v5, m5 = C.case('disc_and_box')                      # 96 x 128
    v3, m3 = C.case('l_top')                             # 33 x 47, padded into a 96 x 128 image (still on the top border)
    va, ma = C.smooth(96, 128, 11), np.zeros((96, 128), bool)
    va[:33, :47], ma[:33, :47] = v3, m3
    ve = C.smooth(96, 128, 12)
    vf = C.smooth(96, 128, 13)
    vf[5, 5] = np.nan
    V = np.stack([va, v5, ve, vf])
    M = np.stack([ma, m5, np.zeros((96, 128), bool), np.ones((96, 128), bool)])
    got, info = fill(cuda, V, M)
    for n in range(4):
        one, i1 = fill(cuda, V[n:n + 1], M[n:n + 1])
        assert np.array_equal(bits(one[0]), bits(got[n])), n
        for k in info:
            assert np.array_equal(info[k][n:n + 1], i1[k], equal_nan=(k == 'residual')), (n, k)
    again, info2 = fill(cuda, V, M)
    assert np.array_equal(bits(again), bits(got))
    for k in info:
        assert np.array_equal(info[k], info2[k], equal_nan=(k == 'residual')), k
    print('batch: iterations', info['iterations'].tolist(), 'unknowns', info['unknowns'].tolist())
    assert info['iterations'][0] > 0 and info['iterations'][1] > 0 and info['iterations'][0] != info['iterations'][1]
    assert np.array_equal(bits(got[2]), bits(ve)) and info['iterations'][2] == 0 and info['unknowns'][2] == 0
    assert info['converged'][2] and not info['singular'][2]
    assert np.array_equal(bits(got[3]), bits(vf)) and info['singular'][3] and not info['converged'][3]
    assert info['iterations'][3] == 0 and info['unknowns'][3] == 96 * 128
    assert info['singular'].tolist() == [False, False, False, True] and info['converged'].tolist() == [True, True, True, False]
    # the padded and the two-hole image: still the fp64 solve
    for n, name in ((0, 'batch_l_top_padded'), (1, 'disc_and_box')):
        _, _, U, f64, e32, _, _ = reference(name, V[n].copy(), M[n].copy())
        assert np.abs(got[n].astype(np.float64) - f64)[U].max() <= 4.0 * e32
    empty, i0 = ops.harmonic_fill(torch.empty((0, 7, 9), device=cuda), torch.empty((0, 7, 9), device=cuda, dtype=torch.bool))
    assert tuple(empty.shape) == (0, 7, 9) and all(len(i0[k]) == 0 for k in ('unknowns', 'iterations', 'residual', 'converged', 'singular'))


# ---- 5. the iteration cap -------------------------------------------------------------------------------------------------------

def test_max_iters_returns_unconverged(cuda):
    v, m = C.case('band')
    got, info = fill(cuda, v[None], m[None], max_iters=3)
    assert not info['converged'][0] and info['iterations'][0] == 3 and not info['singular'][0]
    assert np.isfinite(got).all() and np.array_equal(bits(got[0])[~m], bits(v)[~m])
    got, info = fill(cuda, v[None], m[None], max_iters=3, check_every=2)
    assert not info['converged'][0] and info['iterations'][0] == 3


# ---- 6. dilation ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rounds', [0, 1, 3])
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 47), (64, 130)])
def test_dilation_equals_restatement(shape, rounds, cuda):
    H, W = shape
    rs = np.random.RandomState(H * 131 + W)
    border = np.zeros(shape, bool)
    border[0, W // 2] = border[H - 1, W // 3] = border[H // 2, 0] = border[H // 3, W - 1] = True     # every border
    corner = np.zeros(shape, bool)
    corner[H - 1, W - 1] = True
    M = np.stack([border, rs.rand(H, W) < 0.03, np.zeros(shape, bool), np.ones(shape, bool), corner])
    src = torch.from_numpy(M).to(cuda)
    got = ops.mask_dilate2d(src, rounds)
    assert got.dtype == torch.bool and got.data_ptr() != src.data_ptr() and torch.equal(src.cpu(), torch.from_numpy(M))
    assert np.array_equal(got.cpu().numpy(), R.dilate(M, rounds))
    assert tuple(ops.mask_dilate2d(src[:0], rounds).shape) == (0, H, W)


# ---- 7. the dataset's rasters -------------------------------------------------------------------------------------------------

def test_fixture_rasters_reproduce_the_dataset_inside_the_masks(cuda):
    z = np.load(FIXTURE, allow_pickle=False)
    d = z['depths'].astype(np.float32) / np.float32(255.)
    m = z['masks'].astype(bool)
    assert d.shape == (30, 141, 252)
    got, info = fill(cuda, d, m)
    assert info['converged'].all() and not info['singular'].any()
    rms = lambda f, n: float(np.sqrt(((f[m[n]].astype(np.float64) - d[n][m[n]]) ** 2).mean()) * 255.0)
    gpu = np.array([rms(got[n], n) for n in range(30)])
    ref = np.array([rms(R.solve(d[n], m[n])[0], n) for n in range(30)])
    ring = np.array([rms(R.ring_mean_fill(d[n], m[n]), n) for n in range(30)])
    print(f'fixture: in-mask RMS / 255: gpu mean {gpu.mean():.4f} worst {gpu.max():.4f}, fp64 mean {ref.mean():.4f} worst '
          f'{ref.max():.4f}, ring mean {ring.mean():.4f}; iterations {info["iterations"].min()}..{info["iterations"].max()}')
    assert abs(ref.mean() - 1.366) <= 1e-3 and abs(ref.max() - 1.954) <= 1e-3 and abs(ring.mean() - 8.786) <= 1e-3
    assert np.abs(gpu - ref).max() <= 1e-3
    assert abs(gpu.mean() - 1.366) <= 1e-3 and abs(gpu.max() - 1.954) <= 1e-3


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def mlp(cuda):
    """The seeded 8 x 256 pair with a density head that renders something (the construction of tests/test_region.py, written
    again): alpha_linear rescaled to sigma' = 4 (sigma - median) / std over the camera's sample points."""
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    sel = torch.from_numpy(np.random.RandomState(99).randint(0, bench.H * bench.W, 2000)).to(cuda)
    rows = ops.ray_rows_from_pose(bench.orbit_pose(0, cuda), bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR, sel=sel)
    z = ops.stratified_z(rows, 64, True)
    pts = (rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    dirs = rows[:, None, 8:11].expand(-1, 64, -1).reshape(-1, 3).contiguous()
    for net, seed in ((te['network_fn'], 1), (te['network_fine'], 2)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
        with torch.no_grad():
            sigma = net.query_points(pts, dirs)[:, 3]
            scale = 4.0 / float(sigma.std())
            net.alpha_linear.bias.copy_((net.alpha_linear.bias - sigma.median()) * scale)
            net.alpha_linear.weight.mul_(scale)
        net.invalidate_packed()
    assert te['N_samples'] == 64 and te['N_importance'] == 64
    return te


def test_prepare_depths_end_to_end(mlp, cuda):
    H, W = 24, 32
    focal = bench.FOCAL * W / bench.W
    poses = torch.stack([bench.orbit_pose(0, cuda)[:3, :4], bench.orbit_pose(2, cuda)[:3, :4]])
    masks = np.zeros((2, H, W), bool)
    masks[0, 6:15, 9:22] = True
    masks[1, 8:18, 5:17] = True
    disp = prepare.render_disparities(mlp, (H, W, focal), poses, bench.NEAR, bench.FAR)
    assert disp.shape == (2, H, W) and disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous()
    with torch.no_grad():
        for n in range(2):
            want = run.render(H, W, focal, chunk=1 << 15, c2w=poses[n], **dict(mlp, near=bench.NEAR, far=bench.FAR))[1]
            assert torch.equal(disp[n].view(torch.int32), want.view(torch.int32))
    assert float(disp[torch.isfinite(disp)].std()) > 0
    for dilate in (0, 2):
        out = prepare.prepare_depths(mlp, (H, W, focal), poses, masks, bench.NEAR, bench.FAR, dilate=dilate)
        assert sorted(out) == ['disp', 'filled', 'info', 'masks']
        assert torch.equal(out['disp'].view(torch.int32), disp.view(torch.int32))
        filled_set = out['masks'].cpu().numpy()
        assert filled_set.dtype == bool and np.array_equal(filled_set, R.dilate(masks, dilate))
        d, f = disp.cpu().numpy(), out['filled'].cpu().numpy()
        unknown = filled_set | ~np.isfinite(d)               # a non-finite rendered disparity is a hole too
        assert np.array_equal(bits(f)[~unknown], bits(d)[~unknown]) and np.isfinite(f).all()
        assert out['info']['converged'].all() and np.array_equal(out['info']['unknowns'], unknown.sum((1, 2)))
        for n in range(2):
            _, _, U, f64, e32, _, bound = reference(f'e2e_{dilate}_{n}', d[n].copy(), filled_set[n].copy())
            err = float(np.abs(f[n].astype(np.float64) - f64)[U].max())
            print(f'end to end, dilate {dilate}, view {n}: gpu error {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}')
            assert err <= bound
    # a view with nothing to interpolate from is refused; an unconverged one is named
    with pytest.raises(ValueError, match='views \\[1\\]'):
        prepare.prepare_depths(mlp, (H, W, focal), poses, np.stack([masks[0], np.ones((H, W), bool)]), bench.NEAR, bench.FAR)
    with pytest.raises(RuntimeError, match='views \\[0, 1\\]'):
        prepare.prepare_depths(mlp, (H, W, focal), poses, masks, bench.NEAR, bench.FAR, max_iters=1)
    out = prepare.prepare_depths(mlp, (H, W, focal), poses, masks, bench.NEAR, bench.FAR, max_iters=1, allow_unconverged=True)
    assert not out['info']['converged'].any() and out['info']['iterations'].tolist() == [1, 1]
