"""Gradient-domain (Poisson) blending on the GPU (csrc/harmonic.hip's poisson_init_kernel, ops.poisson_fill,
prepare.propagate_reference(blend='poisson')) against the restatement tests/poisson_numpy.py.

The yardstick is tests/test_prepare.py's: the fp64 direct solve of the same linear system; per case
max |u_gpu - u_fp64| <= 4 * e32, e32 = the max error of the restatement's own fp32 conjugate-gradient run on that case against
the fp64 solve, computed here (the factor 4 covers a different summation order), and never above max |v_K| / 2550, a tenth of
the 8-bit step of the file format.  Every test prints the figures it asserts on.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harmonic_cases as C                               # noqa: E402
import harmonic_numpy as R                               # noqa: E402
import poisson_cases as PC                               # noqa: E402
import poisson_numpy as P                                # noqa: E402
import warp_numpy as WN                                  # noqa: E402

from mvip_nerf_amd import ops, prepare                   # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, v=None, m=None, g=None, l=None):
    """(v, m, g, l, U, fp64 solve, e32, iterations of the fp32 restatement) of a case, computed once and left unchanged."""
    if name not in _REF:
        if v is None:
            v, m, g, l = PC.case(name)
        U = R.unknown_set(v, m)
        f64, singular = P.solve(v, m, g, l)
        assert not singular
        c32, it32, ok = P.cg32(v, m, g, l)
        assert ok
        e32 = float(np.abs(c32.astype(np.float64) - f64)[U].max())
        for a in (v, m, g, l, U, f64):
            a.setflags(write=False)
        _REF[name] = (v, m, g, l, U, f64, e32, it32)
    return _REF[name]


def fill(cuda, v, m, g, l, **kw):
    t = lambda a: torch.from_numpy(np.array(a)).to(cuda)             # copies: the cached cases are read-only
    out, info = ops.poisson_fill(t(v), t(m), t(g), t(l), **kw)
    assert out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
    return out.cpu().numpy(), info


def harmonic(cuda, v, m, **kw):
    out, info = ops.harmonic_fill(torch.from_numpy(np.array(v)).to(cuda), torch.from_numpy(np.array(m)).to(cuda), **kw)
    return out.cpu().numpy(), info


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_info(a, b):
    assert sorted(a) == sorted(b) == ['converged', 'iterations', 'residual', 'singular', 'unknowns']
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=(k == 'residual')), k


# ---- 1. no guided edge: the harmonic fill, bit for bit ---------------------------------------------------------------------------

def test_unguided_equals_harmonic_fill_bit_for_bit(cuda):
    cases = PC.unguided_masks()
    V, M = np.stack([v for v, _ in cases.values()]), np.stack([m for _, m in cases.values()])
    assert V.shape == (5, 37, 70)
    want, winfo = harmonic(cuda, V, M)
    assert winfo['converged'].all() and (winfo['iterations'] > 0).all()
    rs = np.random.RandomState(3)
    G = rs.rand(*V.shape).astype(np.float32)
    labelled = np.stack([PC.ring_labels(m) for m in M])
    for what, g, l in (('labels -1', G, np.full(V.shape, -1, np.int32)), ('guide NaN', np.full_like(G, np.nan), labelled),
                       ('labels all different', G, np.arange(V.size, dtype=np.int32).reshape(V.shape))):
        got, info = fill(cuda, V, M, g, l)
        assert np.array_equal(bits(got), bits(want)), what
        same_info(info, winfo)
    print('unguided:', list(cases), 'iterations', winfo['iterations'].tolist())
    got, info = fill(cuda, V, M, G, labelled)                # and the guide does something
    assert not np.array_equal(bits(got), bits(want))


# ---- 2. the fill against the fp64 direct solve of the restatement ----------------------------------------------------------------

@pytest.mark.parametrize('name', PC.SOLVED)
def test_fill_equals_fp64_direct_solve(name, cuda):
    v, m, g, l, U, f64, e32, it32 = reference(name)
    got, info = fill(cuda, v[None], m[None], g[None], l[None])
    got = got[0]
    err = float(np.abs(got.astype(np.float64) - f64)[U].max())
    ceiling = float(np.abs(v[~U]).max()) / 2550.0
    print(f'{name}: unknowns {int(U.sum())}, gpu error {err:.3e}, e32 {e32:.3e}, 4 e32 {4 * e32:.3e}, ceiling {ceiling:.3e}, '
          f'iterations gpu {int(info["iterations"][0])} / restatement {it32}, true residual {float(info["residual"][0]):.3e}')
    assert info['unknowns'][0] == U.sum() and info['converged'][0] and not info['singular'][0]
    assert U.sum() == m.sum() + (name == 'value_nonfinite')
    assert err <= 4.0 * e32
    assert err <= ceiling
    assert np.array_equal(bits(got)[~U], bits(v)[~U]) and np.isfinite(got).all()
    # each case is what it says: the harmonic fill of the same values is far from it
    h64, _ = R.solve(v, m)
    assert np.abs(h64 - f64)[U].max() > 1000 * 4.0 * e32


def test_offset_is_reproduced(cuda):
    v, m, g, l, U, f64, e32, _ = reference('offset')
    got, _ = fill(cuda, v[None], m[None], g[None], l[None])
    err = float(np.abs(got[0].astype(np.float64) - (g.astype(np.float64) + float(PC.OFFSET)))[U].max())
    print(f'offset: gpu against g + c {err:.3e}, bound {4 * e32 + 1e-6:.3e} (e32 {e32:.3e})')
    assert err <= 4.0 * e32 + 1e-6


# ---- 3. batches ------------------------------------------------------------------------------------------------------------------

def test_batch_equals_single_calls_bit_for_bit(cuda):
    v, m, g, l = PC.case('step_two_labels')
    v2, m2 = PC.unguided_masks()['disc_over_tile_edges']
    v3, v4 = C.smooth(PC.H, PC.W, 41), C.smooth(PC.H, PC.W, 42)
    none = np.full((PC.H, PC.W), -1, np.int32)
    V, M = np.stack([v, v2, v3, v4]), np.stack([m, m2, np.zeros_like(m), np.ones_like(m)])
    G, L = np.stack([g, g, g, g]), np.stack([l, none, l, l])         # guided, unguided, empty mask, fully masked (singular)
    got, info = fill(cuda, V, M, G, L)
    for n in range(4):
        one, i1 = fill(cuda, V[n:n + 1], M[n:n + 1], G[n:n + 1], L[n:n + 1])
        assert np.array_equal(bits(one[0]), bits(got[n])), n
        for k in info:
            assert np.array_equal(info[k][n:n + 1], i1[k], equal_nan=(k == 'residual')), (n, k)
    again, info2 = fill(cuda, V, M, G, L)
    assert np.array_equal(bits(again), bits(got))
    same_info(info, info2)
    print('batch: iterations', info['iterations'].tolist(), 'unknowns', info['unknowns'].tolist())
    assert info['iterations'][0] > 0 and info['iterations'][1] > 0
    h, hinfo = harmonic(cuda, V[1:2], M[1:2])
    assert np.array_equal(bits(got[1]), bits(h[0])) and info['iterations'][1] == hinfo['iterations'][0]
    assert np.array_equal(bits(got[2]), bits(v3)) and info['iterations'][2] == 0 and info['unknowns'][2] == 0
    assert np.array_equal(bits(got[3]), bits(v4)) and info['iterations'][3] == 0 and info['unknowns'][3] == PC.H * PC.W
    assert info['singular'].tolist() == [False, False, False, True] and info['converged'].tolist() == [True, True, True, False]
    _, _, _, _, U, f64, e32, _ = reference('step_two_labels')
    assert np.abs(got[0].astype(np.float64) - f64)[U].max() <= 4.0 * e32
    empty, i0 = ops.poisson_fill(torch.empty((0, 7, 9), device=cuda), torch.empty((0, 7, 9), device=cuda, dtype=torch.bool),
                                 torch.empty((0, 7, 9), device=cuda), torch.empty((0, 7, 9), device=cuda, dtype=torch.int32))
    assert tuple(empty.shape) == (0, 7, 9) and all(len(i0[k]) == 0 for k in ('unknowns', 'iterations', 'residual', 'converged', 'singular'))


def test_max_iters_returns_unconverged(cuda):
    v, m, g, l = PC.case('offset')
    got, info = fill(cuda, v[None], m[None], g[None], l[None], max_iters=1)
    assert not info['converged'][0] and info['iterations'][0] == 1 and not info['singular'][0]
    assert np.isfinite(got).all() and np.array_equal(bits(got[0])[~m], bits(v)[~m])


# ---- 4. propagate_reference(blend='poisson') ---------------------------------------------------------------------------------------

SCENE_OFFSET = np.float32(0.1)


def scene():
    """Four cameras side by side in front of the textured plane z = -3 (40 x 72, f = 60); views 0 and 3 are the references, their
    reference images the scene's plus SCENE_OFFSET.  View 1's mask reaches the top border, where its raised camera sees what no
    reference does (holes); both masks are wide enough that a few columns leave the nearer reference and take the other."""
    H, W, f = 40, 72, 60.0
    poses = np.stack([WN.pose((0, 0, 0), (x, y, 0.0)) for x, y in ((-0.8, 0.0), (-0.2, 0.25), (0.2, 0.0), (0.8, 0.0))])
    disp = np.stack([WN.plane_disparity(p, H, W, f, (0, 0, 1.0), -3.0) for p in poses]).astype(np.float32)
    img = []
    for p in poses:
        o, d = WN.pixel_rays(p, H, W, f)
        X, Y = o[0] - 3.0 * d[..., 0] / d[..., 2], o[1] - 3.0 * d[..., 1] / d[..., 2]
        img.append(np.stack([.5 + .25 * np.sin(a * X + b * Y + c) * np.cos(.7 * a * Y - c)
                             for a, b, c in ((2.1, 1.3, .3), (1.1, 2.7, 1.1), (1.7, 1.9, 2.3))], -1))
    img = np.stack(img).astype(np.float32)
    masks = np.zeros((4, H, W), bool)
    masks[1, 0:22, 4:68] = True
    masks[2, 12:34, 4:68] = True
    masks[3, 5:15, 30:50] = True                             # a reference's own mask: not warped into, not blended
    refs = [0, 3]
    return img, masks, disp, poses, f, refs, (img[refs] + SCENE_OFFSET).astype(np.float32)


@pytest.mark.parametrize('fill_kind', ['harmonic', 'exemplar'])
def test_propagate_reference_poisson(fill_kind, cuda):
    img, masks, disp, poses, f, refs, ref_images = scene()
    N, H, W = masks.shape
    call = lambda **kw: prepare.propagate_reference(img, masks, disp, poses, f, refs, ref_images=ref_images, fill=fill_kind, **kw)
    cpu = lambda r: {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
    before = cpu(call())
    out = cpu(call(blend='poisson'))
    after = cpu(call(blend='none'))
    # blend='none' is untouched by the call in between, and keeps its keys
    assert sorted(before) == sorted(after) == ['coverage', 'holes', 'images', 'info', 'resid', 'source']
    for k in ('images', 'resid', 'source', 'holes', 'coverage'):
        assert np.array_equal(before[k].view(np.int32) if before[k].dtype == np.float32 else before[k],
                              after[k].view(np.int32) if after[k].dtype == np.float32 else after[k]), k
    assert sorted(out) == ['coverage', 'holes', 'images', 'info', 'pasted', 'resid', 'source']
    # the report on the masks is blend='none''s; so is the pasted composite
    for k in ('source', 'holes', 'coverage'):
        assert np.array_equal(out[k], before[k]), k
    assert np.array_equal(bits(out['resid']), bits(before['resid'])) and np.array_equal(bits(out['pasted']), bits(before['images']))
    got, source, holes = out['images'], out['source'], out['holes']
    others = [1, 2]
    assert holes[1].sum() > 100 and not holes[refs].any()
    assert all(((source[n] == k) & masks[n]).sum() > 50 for n in others for k in (0, 1))      # two references meet in each mask
    for n in others:                                         # outside the masks: the input, bit for bit
        assert np.array_equal(bits(got[n])[~masks[n]], bits(img[n])[~masks[n]])
    for k, v in enumerate(refs):                             # a reference view: its reference image
        assert np.array_equal(bits(got[v]), bits(ref_images[k]))
    assert len(out['info']['iterations']) == 3 * N and out['info']['converged'][[3, 4, 5, 6, 7, 8]].all()
    assert (out['info']['unknowns'].reshape(N, 3) == np.array([0, masks[1].sum(), masks[2].sum(), 0])[:, None]).all()
    # the seam: the step across the mask's boundary edges falls from the pasted composite's towards the image's own
    for n in others:
        pasted, blended, own = (P.boundary_step(x[n], masks[n]) for x in (out['pasted'], got, img))
        rms = lambda x: float(np.sqrt(((x[n].astype(np.float64) - img[n]) ** 2)[masks[n]].mean()))
        print(f'{fill_kind}, view {n}: boundary step pasted {pasted:.4f}, blended {blended:.4f}, the image\'s own {own:.4f}; in-mask RMS '
              f'against the image pasted {rms(out["pasted"]):.4f}, blended {rms(got):.4f}')
        assert blended < pasted
    # the level: the restatement on the same guide and labels (the warp over the dilated masks, the exemplar holes under their
    # own label), the view's own pixels as the boundary
    wide = R.dilate(masks, 1)
    wide[refs] = False
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    order = prepare.reference_order(poses, refs)
    rgb, index, _ = ops.warp_views(t(disp), t(poses), t(wide), t(ref_images), t(disp[refs]), t(poses[refs]), f, order=t(order))
    guide, labels = rgb.cpu().numpy(), index.cpu().numpy()
    assert np.array_equal(labels[masks & ~np.isin(np.arange(N), refs)[:, None, None]], source[masks & ~np.isin(np.arange(N), refs)[:, None, None]])
    if fill_kind == 'exemplar':
        guide[holes], labels[holes] = out['pasted'][holes], len(refs)
    for n in others:
        for c in range(3):
            v, g = np.ascontiguousarray(img[n, :, :, c]), np.ascontiguousarray(guide[n, :, :, c])
            _, _, _, _, U, f64, e32, it32 = reference(f'scene_{fill_kind}_{n}_{c}', v, masks[n].copy(), g, labels[n].copy())
            err = float(np.abs(got[n, :, :, c].astype(np.float64) - f64)[U].max())
            print(f'{fill_kind}, view {n}, channel {c}: gpu error {err:.3e}, e32 {e32:.3e}, iterations gpu '
                  f'{int(out["info"]["iterations"][3 * n + c])} / restatement {it32}')
            assert err <= 4.0 * e32 and err <= float(np.abs(v[~U]).max()) / 2550.0
    # an unconverged blend is named
    with pytest.raises(RuntimeError, match='did not converge'):
        call(blend='poisson', max_iters=1)
    loose = call(blend='poisson', max_iters=1, allow_unconverged=True)
    assert not loose['info']['converged'][[3, 4, 5, 6, 7, 8]].any()
