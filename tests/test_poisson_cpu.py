"""Gradient-domain (Poisson) blending without a GPU: the restatement tests/poisson_numpy.py (no guided edge = the harmonic
right-hand side bit for bit, a constant offset is reproduced, the label rule does something), the refusals of
ops.poisson_fill, mvip_poisson_init and prepare.propagate_reference(blend=...), and the tool's --help."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harmonic_numpy as R                               # noqa: E402
import poisson_cases as PC                               # noqa: E402
import poisson_numpy as P                                # noqa: E402

from mvip_nerf_amd import _lib, ops, prepare             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
P0 = None            # NULL


def raw(name, *args):
    return getattr(_lib.load(), name)(*args)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['offset', 'two_borders', 'value_nonfinite'])
def test_no_guided_edge_is_the_harmonic_right_hand_side(name):
    v, m, g, l = PC.case(name)
    _, b, _, U, b32 = R.system(v, m)
    assert b32.size > 0 and np.abs(b32).max() > 0
    for what, gg, ll in (('labels -1', g, np.full_like(l, -1)), ('guide NaN', np.full_like(g, np.nan), l),
                         ('guide inf', np.full_like(g, np.inf), l)):
        A2, b2, deg2, U2, b32_2 = P.system(v, m, gg, ll)
        assert np.array_equal(U2, U) and np.array_equal(b2, b), what
        assert b32_2.dtype == np.float32 and np.array_equal(bits(b32_2), bits(b32)), what
    t, t32 = P.guidance(U, g, l)                             # and with the guide it is another one
    assert np.abs(t).max() > 0 and np.abs(t32).max() > 0 and np.abs(t - t32).max() <= 4 * 2.0 ** -24


def test_single_labels_guide_only_their_own_edges():
    v, m, g, l = PC.case('offset')
    U = R.unknown_set(v, m)
    l2 = l.copy()
    ys, xs = np.nonzero(U)
    k = int(np.nonzero((ys == 18) & (xs == 40))[0][0])
    l2[18, 40] = 7                                           # a pixel of its own source: its four edges fall back
    t, _ = P.guidance(U, g, l)
    t2, _ = P.guidance(U, g, l2)
    assert t[k] != 0 and t2[k] == 0
    changed = np.nonzero(t != t2)[0]
    assert set(zip(ys[changed], xs[changed])) == {(18, 40), (17, 40), (19, 40), (18, 39), (18, 41)}


def test_offset_is_reproduced():
    v, m, g, l = PC.case('offset')
    assert v.shape == (37, 70) and m.sum() > 500
    f64, singular = P.solve(v, m, g, l)
    want = g.astype(np.float64) + float(PC.OFFSET)
    err = float(np.abs(f64 - want)[m].max())
    c32, it, ok = P.cg32(v, m, g, l)
    e32 = float(np.abs(c32.astype(np.float64) - f64)[m].max())
    print(f'offset: fp64 solve against g + c {err:.3e}; fp32 CG {it} iterations, e32 {e32:.3e}')
    assert not singular and ok
    assert err <= 1e-6
    assert np.array_equal(bits(f64.astype(np.float32))[~m], bits(v)[~m])
    # without the guide the same boundary gives a visibly different (harmonic) interior
    h64, _ = R.solve(v, m)
    assert np.abs(h64 - want)[m].max() > 100 * 1e-6


def test_the_label_rule_does_something():
    v, m, g0, _ = PC.case('offset')
    want = g0.astype(np.float64) + float(PC.OFFSET)
    err = {}
    for name in ('step_one_label', 'step_two_labels'):
        v1, m1, g, l = PC.case(name)
        assert np.array_equal(bits(v1), bits(v)) and np.array_equal(m1, m)
        f64, _ = P.solve(v1, m1, g, l)
        err[name] = float(np.abs(f64 - want)[m].max())
    print(f'step of {float(PC.STEP)} in the guide at x = {PC.SPLIT}: error against g + c with one label {err["step_one_label"]:.4f}, '
          f'with two labels {err["step_two_labels"]:.4f}')
    assert err['step_two_labels'] < 0.5 * err['step_one_label']


def test_boundary_step():
    x = np.zeros((5, 6))
    m = np.zeros((5, 6), bool)
    m[0:2, 2:4] = True                                       # on the top border: 2 + 2 + 2 boundary edges
    x[m] = [1.0, 2.0, 3.0, 5.0]
    assert P.boundary_step(x, m) == pytest.approx((1 + 3 + 2 + 5 + 3 + 5) / 6.0)
    assert P.boundary_step(np.stack([x, 2 * x], -1), m) == pytest.approx(1.5 * (1 + 3 + 2 + 5 + 3 + 5) / 6.0)
    assert P.boundary_step(x, np.zeros_like(m)) is None and P.boundary_step(x, np.ones_like(m)) is None


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_poisson_fill_refuses_bad_arguments():
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    v, m, g, l = z(2, 5, 7), z(2, 5, 7, dtype=torch.bool), z(2, 5, 7), z(2, 5, 7, dtype=torch.int32)

    def check(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            ops.poisson_fill(*a, **kw)
    check('GPU', v, m, g, l)                                 # no CPU fallback
    check('GPU', v.numpy(), m.numpy(), g.numpy(), l.numpy())
    check('float32', v.double(), m, g, l)
    check('bool', v, m.to(torch.uint8), g, l)
    check('guide must be torch.float32', v, m, g.double(), l)
    check('labels must be torch.int32', v, m, g, l.long())
    check(r'\[N, H, W\]', v[0], m[0], g[0], l[0])
    check(r'guide must be \[N, H, W\]', v, m, g[0], l)
    check('masks', v, z(2, 5, 8, dtype=torch.bool), g, l)
    check('guide', v, m, z(2, 5, 8), l)
    check('labels', v, m, g, z(2, 6, 7, dtype=torch.int32))
    check('values must be contiguous', z(2, 5, 14)[:, :, ::2], m, g, l)
    check('guide must be contiguous', v, m, z(2, 5, 14)[:, :, ::2], l)
    check('eps', v, m, g, l, eps=1.0)
    check('max_iters', v, m, g, l, max_iters=-1)
    check('check_every', v, m, g, l, check_every=0)
    p = inspect.signature(ops.poisson_fill).parameters
    assert list(p) == ['values', 'masks', 'guide', 'labels', 'eps', 'max_iters', 'check_every']
    assert (p['eps'].default, p['max_iters'].default, p['check_every'].default) == (1e-7, None, 32)


def test_poisson_init_argument_checks():
    assert len(_lib._SIGNATURES['mvip_poisson_init'][1]) == 11
    init = lambda N, H, W, max_act, values=P0, guide=P0, labels=P0, out=P0, ws=P0, state=P0: \
        raw('mvip_poisson_init', values, guide, labels, N, H, W, out, ws, state, max_act, P0)
    for N, H, W in ((2, 0, 47), (2, 33, 0), (-1, 33, 47), (2, 16385, 47), (1 << 40, 33, 47)):       # bad shapes
        assert init(N, H, W, 1) == EINVAL
    assert init(0, 0, 47, 1) == EINVAL                       # a bad shape also with no image
    assert init(0, 33, 47, 1) == OK                          # no image: nothing launched, null operands are fine
    assert init(2, 33, 47, 0) == OK                          # no active tile: nothing launched
    assert init(2, 33, 47, 1) == EINVAL                      # a good shape with null operands
    assert init(2, 33, 47, 4) == EINVAL                      # more active tiles than the image has (3)
    assert init(2, 33, 47, -1) == EINVAL
    # every operand on its own, and out == values.  The pointers are never followed: the checks come before the launch, and
    # each of these calls fails one.
    a = dict(values=1 << 12, guide=2 << 12, labels=3 << 12, out=4 << 12, ws=5 << 12, state=6 << 12)
    for k in a:
        assert init(2, 33, 47, 1, **dict(a, **{k: P0})) == EINVAL, k
    assert init(2, 33, 47, 1, **dict(a, out=a['values'])) == EINVAL


def test_propagate_reference_refuses_a_bad_blend():
    img, msk = np.zeros((2, 4, 4, 3), np.float32), np.zeros((2, 4, 4), bool)
    disp, poses = np.ones((2, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)
    with pytest.raises(ValueError, match='blend'):
        prepare.propagate_reference(img, msk, disp, poses, 1.0, [0], blend='laplace')
    for fill in ('none', False):
        with pytest.raises(ValueError, match='fill'):
            prepare.propagate_reference(img, msk, disp, poses, 1.0, [0], blend='poisson', fill=fill)
    assert inspect.signature(prepare.propagate_reference).parameters['blend'].default == 'none'


def test_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'propagate_reference.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--blend' in r.stdout and 'poisson' in r.stdout
