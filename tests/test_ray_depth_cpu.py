"""Quantile termination depth without a GPU: the restatement (tests/ray_depth_numpy.py) against hand-computed rays and on
the compositing fixture, the argument checks of mvip_ray_quantile_depth with NULL operands, the binding table, the wrappers'
refusals and keyword defaults, and the tool's --help."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_depth_numpy as R                              # noqa: E402

from mvip_nerf_amd import _lib, mesh, ops, prepare, run  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'render_rays_test.npz')
OK, EINVAL = 0, -1
P0 = None            # NULL


def f32(x):
    return np.float32(x)


def test_two_surfaces_the_median_sits_on_one_the_mean_between():
    z, w = R.hand_rays()
    got = R.quantile_depth(z[:1], w[:1], (0.5,))[0, 0]
    # weights 0.55 / 0.45 at the ends of linspace(2, 6, 8): the median lies in the first interval, at 0.5 / 0.55 of its length
    L = int(np.floor(np.float64(f32(0.5)) * 2.0 ** 40))
    W0 = int(np.floor(np.float64(f32(0.55)) * 2.0 ** 40))
    exact = np.float64(z[0, 0]) + (np.float64(L) / np.float64(W0)) * (np.float64(z[0, 1]) - np.float64(z[0, 0]))
    assert got == f32(exact)
    assert abs(float(got) - (2 + (0.5 / 0.55) * (4 / 7))) < 1e-6
    assert abs(R.expected_depth(z[0], w[0]) - 3.8) < 1e-6                  # where nothing is
    assert R.quantile_depth(z[:1], w[:1], (0.6,))[0, 0] == z[0, 7]         # the far surface: the last sample's own depth


def test_exact_tie_takes_the_whole_interval():
    z, w = R.hand_rays()
    assert R.quantile_depth(z[1:2], w[1:2], (0.5,))[0, 0] == z[1, 2]       # C_1 = Lq: k = 1, f = 1, depth = z_2


def test_last_sample_unreached_levels_and_leading_zeros():
    z, w = R.hand_rays()
    assert (R.quantile_depth(z[2:3], w[2:3], (0.16, 0.5, 0.84)) == z[2, 7]).all()
    got = R.quantile_depth(z[3:4], w[3:4], (0.05, 0.5))                    # acc = 0.1
    assert got[0, 1] == np.inf and z[3, 2] < got[0, 0] < z[3, 3]
    got = R.quantile_depth(z[4:5], w[4:5], (0.25, 0.5, 0.75))[0]           # 0.5 at sample 4, 0.5 at sample 5
    assert got[0] == f32((np.float64(z[4, 4]) + np.float64(z[4, 5])) / 2) and got[1] == z[4, 5]
    assert z[4, 5] < got[2] < z[4, 6]


def test_nan_weight_poisons_its_ray_only():
    z, w = R.hand_rays()
    got = R.quantile_depth(z, w, (0.16, 0.5))
    assert np.isnan(got[5]).all() and not np.isnan(got[:5]).any()
    w[4, 0] = np.inf
    assert np.isnan(R.quantile_depth(z, w, (0.5,))[4]).all()


def test_single_sample_and_clamping():
    assert R.quantile_depth([[3.0]], [[0.7]], (0.5, 0.9)).tolist() == [[3.0, np.inf]]
    # weights above 1 count as 1, below 0 as 0
    z = np.array([[1.0, 2.0, 3.0]], np.float32)
    assert R.quantile_depth(z, [[-5.0, 7.0, 0.0]], (0.5,))[0, 0] == f32(2.5)


def test_fixture_quantiles_are_ordered_and_inside_the_ray():
    fx = np.load(FIXTURE)
    z, w = fx['z_vals'], fx['weights']
    assert z.shape == (64, 128) and np.allclose(w.sum(-1), 1.0, atol=1e-4)
    q = R.quantile_depth(z, w, (0.16, 0.5, 0.84))
    assert np.isfinite(q).all()
    assert (q[:, 0] <= q[:, 1]).all() and (q[:, 1] <= q[:, 2]).all()
    assert (q >= z[:, :1]).all() and (q <= z[:, -1:]).all()


def test_levels_are_checked():
    for bad in ((), (0.0,), (1.0,), (-0.1,), (float('nan'),), (2.0 ** -41,), (0.5,) * 9):
        with pytest.raises(ValueError):
            R.level_units(bad)
        with pytest.raises(ValueError):
            ops._quantile_levels('t', bad)
    assert R.level_units((0.5, 2.0 ** -40)) == [2 ** 39, 1]
    assert list(ops._quantile_levels('t', (0.16, 0.5))) == [float(f32(0.16)), 0.5]


def test_entry_point_argument_checks():
    name = 'mvip_ray_quantile_depth'
    assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == 8 and _lib.ABI_VERSION == 5
    lv = lambda *q: (ctypes.c_float * len(q))(*q)
    raw = lambda B, S, levels, Q: getattr(_lib.load(), name)(P0, P0, B, S, levels, Q, P0, P0)
    half = lv(0.5)
    for B, S in ((-1, 8), (4, 0), (4, -1), (4, 4097), ((2 ** 31 - 1) // 192 + 1, 192), (0, 0), (0, 4097)):
        assert raw(B, S, half, 1) == EINVAL, (B, S)
    for Q in (0, -1, 9):
        assert raw(4, 8, lv(*([0.5] * 9)), Q) == EINVAL, Q
    for q in (0.0, 1.0, -0.5, 1.5, float('nan'), float('inf'), 2.0 ** -41):
        assert raw(4, 8, lv(q), 1) == EINVAL, q
        assert raw(0, 8, lv(0.5, q), 2) == EINVAL, q                       # a bad level also with no ray
    assert raw(4, 8, None, 1) == EINVAL
    assert raw(0, 8, half, 1) == OK and raw(0, 4096, lv(*([0.5] * 8)), 8) == OK      # no ray: nothing launched
    assert raw(4, 8, half, 1) == EINVAL                                    # NULL operands


def test_wrappers_refuse_bad_arguments():
    z = torch.zeros(4, 8)
    with pytest.raises(_lib.MvipError, match='ray_quantile_depth'):
        ops.ray_quantile_depth(z, torch.zeros(4, 7))
    with pytest.raises(_lib.MvipError, match='ray_quantile_depth'):
        ops.ray_quantile_depth(z[0], z[0])
    with pytest.raises(_lib.MvipError, match='ray_quantile_depth'):
        ops.ray_quantile_depth(np.zeros((4, 8)), z)
    with pytest.raises(_lib.MvipError, match='4096'):
        ops.ray_quantile_depth(torch.zeros(1, 4097), torch.zeros(1, 4097))
    for bad in ((), (0.0,), (1.0,), (0.5,) * 9, 0.5):
        with pytest.raises(ValueError, match='level'):
            ops.ray_quantile_depth(z, z, bad)
    with pytest.raises(_lib.MvipError, match='no CPU fallback'):
        ops.ray_quantile_depth(z, z)
    with pytest.raises(ValueError, match='kind'):
        prepare.render_disparities({}, (4, 4, 4.0), torch.zeros(0, 3, 4), 2.0, 6.0, kind='mode')
    with pytest.raises(ValueError, match='kind'):
        prepare.prepare_depths({}, (4, 4, 4.0), torch.zeros(0, 3, 4), np.zeros((0, 4, 4), bool), 2.0, 6.0, kind='mode')
    with pytest.raises(ValueError, match='max_spread'):
        prepare.spread_mask(torch.ones(1, 2, 2, 3), float('nan'))
    with pytest.raises(ValueError, match='depth_q'):
        prepare.spread_mask(torch.ones(1, 2, 2, 2), 0.1)


def test_spread_mask():
    q = torch.tensor([[[[2.0, 2.1, 2.2], [2.0, 4.0, 6.0], [2.0, 3.0, float('inf')], [float('nan'), 3.0, 4.0]]]])
    assert prepare.spread_mask(q, 0.1).tolist() == [[[True, False, False, False]]]
    assert prepare.spread_mask(q, 1.0).tolist() == [[[True, True, False, False]]]


def test_keyword_defaults():
    sig = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items()}
    assert sig(ops.ray_quantile_depth)['levels'] == (0.5,)
    assert sig(run.render_rays)['depth_quantiles'] is None
    assert sig(prepare.render_disparities)['kind'] == 'expected' and sig(prepare.prepare_depths)['kind'] == 'expected'
    assert sig(prepare.render_depth_quantiles)['levels'] == (0.16, 0.5, 0.84) and sig(prepare.render_depth_quantiles)['chunk'] == 1 << 15
    s = sig(mesh.extract_mesh_tsdf)
    assert (s['depth'], s['max_spread'], s['min_agree'], s['max_violated']) == ('expected', None, None, None)


@pytest.mark.parametrize('tool,opts', [
    ('depth_quality.py', ('--iters', '--views', '--max-spread', '--sweep', '--tol', '--out')),
    ('extract_mesh.py', ('--tsdf-depth', '--max-spread', '--min-agree', '--max-violated')),
    ('prepare_depths.py', ('--depth',)),
])
def test_tool_help(tool, opts):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), '--help'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for opt in opts:
        assert opt in r.stdout, opt
