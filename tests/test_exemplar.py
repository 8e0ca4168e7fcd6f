"""Exemplar-based inpainting on the GPU (csrc/exemplar.hip, ops.exemplar_fill, prepare.inpaint_views and
propagate_reference(fill='exemplar')) against the numpy restatement (tests/exemplar_numpy.py).  Everything after the
quantisation is integer arithmetic, so every comparison is bit-equality: the filled image, the field and the energy.  No
tolerance applies anywhere in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exemplar_numpy as R                               # noqa: E402

from mvip_nerf_amd import ops, prepare                   # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene1_small.npz')
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
KEYS = ('targets', 'sources', 'levels', 'energy', 'singular')


def picture(H, W, seed=0):
    """A smooth ramp, a grid and noise in fp32, with a few values outside 0..1 (they are clipped)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.5 + 0.4 * np.sin(x / 3.0) * np.cos(y / 4.0), (x + y) / (H + W), ((x // 4 + y // 5) % 2) * 0.6 + 0.2], -1)
    img = (img + rs.uniform(-0.1, 0.1, (H, W, 3))).astype(np.float32)
    img[1, 1], img[2, 2] = (-0.25, 1.5, 0.5), (1.0, 0.0, 1.25)
    return img


def hole(kind, H, W):
    m = np.zeros((H, W), bool)
    if kind == 'interior':
        m[H // 3:H // 3 + 6, W // 3:W // 3 + 8] = True
    elif kind == 'edge':
        m[0:5, W // 2:W // 2 + 7] = True
    elif kind == 'corner':
        m[H - 6:, W - 7:] = True
    elif kind == 'two':
        m[4:8, 5:10] = True
        m[H - 12:H - 8, W - 14:W - 8] = True
    elif kind == 'crossing':                             # 12 x 12: more than 256 targets, and it spans a 1024-pixel group where H W > 1024
        m[H // 2 - 6:H // 2 + 6, W // 2 - 6:W // 2 + 6] = True
    elif kind == 'pixel':
        m[H // 2, W // 3] = True
    return m


def gpu_fill(cuda, images, masks, sources=None, **kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    out, info = ops.exemplar_fill(t(images), t(masks), sources=t(sources), **kw)
    torch.cuda.synchronize()
    info = dict(info, nnf=info['nnf'].cpu().numpy())
    return out.cpu().numpy(), info


def assert_same(got, want, what=''):
    (g, gi), (w, wi) = got, want
    for k in KEYS:
        assert np.array_equal(gi[k], wi[k]), (what, k, gi[k], wi[k])
    assert np.array_equal(gi['nnf'], wi['nnf']), (what, 'nnf differs at', int((gi['nnf'] != wi['nnf']).any(-1).sum()))
    assert np.array_equal(bits(g), bits(w)), (what, 'image differs at', int((bits(g) != bits(w)).any(-1).sum()))


@pytest.mark.parametrize('kind', ['interior', 'edge', 'corner', 'two', 'crossing', 'pixel'])
@pytest.mark.parametrize('shape', [(37, 53), (29, 29), (120, 136)])
def test_equals_the_restatement(shape, kind, cuda):
    H, W = shape
    img, m = picture(H, W, seed=H)[None], hole(kind, H, W)[None]
    want = R.fill(img, m, seed=5)
    got = gpu_fill(cuda, img, m, seed=5)
    assert want[1]['levels'][0] == {37: 1, 29: 1, 120: 3}[H] and want[1]['targets'][0] > 0 and not want[1]['singular'][0]
    assert_same(got, want, f'{shape} {kind}')
    assert np.array_equal(bits(got[0])[~m], bits(img)[~m])
    inside = got[0][m]
    assert np.array_equal(bits(inside), bits(np.rint(inside * 255).astype(np.float32) / np.float32(255)))       # k / 255


def batch_case():
    H, W = 37, 53
    img = np.stack([picture(H, W, 1), picture(H, W, 2), picture(H, W, 3)])
    m = np.zeros((3, H, W), bool)
    m[0] = hole('interior', H, W)
    m[2, 3:-3, 3:-3] = True                               # a 3-pixel rim: no 7 x 7 patch is free of the hole
    return img, m


def test_batch_equals_single_calls(cuda):
    img, m = batch_case()
    got = gpu_fill(cuda, img, m, seed=2)
    assert_same(got, R.fill(img, m, seed=2), 'batch')
    assert got[1]['singular'].tolist() == [False, False, True] and got[1]['levels'].tolist() == [1, 1, 0]
    assert got[1]['targets'][1] == 0 and got[1]['energy'][1] == 0 and got[1]['sources'][2] == 0
    assert np.array_equal(bits(got[0][1:]), bits(img[1:])) and (got[1]['nnf'][1:] == -1).all()   # the empty and the singular: unchanged
    for n in range(3):
        one = gpu_fill(cuda, img[n:n + 1], m[n:n + 1], seed=2)
        assert np.array_equal(bits(one[0][0]), bits(got[0][n])) and np.array_equal(one[1]['nnf'][0], got[1]['nnf'][n])
        assert all(one[1][k][0] == got[1][k][n] for k in KEYS)
    # no image, and no hole at all
    e = gpu_fill(cuda, img[:0], m[:0])
    assert e[0].shape == (0, 37, 53, 3) and e[1]['nnf'].shape == (0, 37, 53, 2) and all(len(e[1][k]) == 0 for k in KEYS)
    none = gpu_fill(cuda, img, np.zeros_like(m))
    assert np.array_equal(bits(none[0]), bits(img)) and not none[1]['targets'].any() and (none[1]['nnf'] == -1).all()


@pytest.mark.parametrize('patch', [5, 9])
def test_patch_sizes(patch, cuda):
    img, m = picture(37, 53, 4)[None], hole('interior', 37, 53)[None]
    assert_same(gpu_fill(cuda, img, m, patch=patch, seed=1), R.fill(img, m, patch=patch, seed=1), f'patch {patch}')


def test_sources_restrict_the_exemplars(cuda):
    img, m = picture(37, 53, 6)[None], hole('interior', 37, 53)[None]
    src = np.zeros((1, 37, 53), bool)
    src[:, :, :26] = True
    got = gpu_fill(cuda, img, m, sources=src, seed=3)
    assert_same(got, R.fill(img, m, sources=src, seed=3), 'sources')
    nnf = got[1]['nnf'][0]
    on = nnf[..., 0] >= 0
    assert on.sum() == got[1]['targets'][0] and nnf[..., 1][on].max() + 3 < 26           # every exemplar patch lies in the left half
    assert got[1]['sources'][0] < gpu_fill(cuda, img, m, seed=3)[1]['sources'][0]


def test_non_finite_pixels_join_the_hole(cuda):
    img, m = picture(37, 53, 7)[None], hole('interior', 37, 53)[None]
    img[0, 30, 40, 1], img[0, 8, 45, 0] = np.nan, np.inf
    got = gpu_fill(cuda, img, m, seed=4)
    assert_same(got, R.fill(img, m, seed=4), 'non-finite')
    assert np.isfinite(got[0]).all() and got[1]['nnf'][0, 30, 40, 0] >= 0
    m2 = m.copy()
    m2[0, 30, 40] = m2[0, 8, 45] = True
    assert got[1]['targets'][0] == gpu_fill(cuda, np.nan_to_num(img, posinf=0.0), m2, seed=4)[1]['targets'][0]


def test_periodic_texture_is_reproduced_exactly(cuda):
    t, m = R.periodic_textures()[0][None], R.periodic_holes()[None]
    got = gpu_fill(cuda, t, m, seed=1)
    assert_same(got, R.fill(t, m, seed=1), 'periodic')
    assert got[1]['levels'][0] == 2 and got[1]['energy'][0] == 0
    assert np.array_equal(bits(got[0]), bits(t))


def test_two_calls_are_bit_equal(cuda):
    img, m = picture(120, 136, 8)[None], hole('crossing', 120, 136)[None]
    a, b = gpu_fill(cuda, img, m, seed=9), gpu_fill(cuda, img, m, seed=9)
    assert_same(a, b, 'repeat')
    c = gpu_fill(cuda, img, m, seed=10)
    assert not np.array_equal(a[1]['nnf'], c[1]['nnf'])


def fixture(views):
    z = np.load(FIXTURE, allow_pickle=False)
    P = z['poses']
    H, W = z['images'].shape[1:3]
    return (z['images'][views].astype(np.float32) / np.float32(255.), z['depths'][views].astype(np.float32) / np.float32(255.),
            z['masks'][views].astype(bool), np.ascontiguousarray(P[views][:, :, :4]), float(P[0, 2, 4]) * W / float(P[0, 1, 4]))


def test_propagate_reference_fills(cuda):
    img, disp, masks, pose, focal = fixture([0, 1, 5, 15])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    refs = [0]
    # by hand: the warp, then the fill of what no reference sees
    order = t(prepare.reference_order(pose, refs))
    wm = masks.copy()
    wm[refs] = False
    rgb, source, _ = ops.warp_views(t(disp), t(pose), t(wm), t(img[refs]), t(disp[refs]), t(pose[refs]), focal, order=order, tol=0.05)
    base = torch.where((source >= 0)[..., None], rgb, t(img))
    base[0] = t(img[0])
    source[0] = torch.where(t(masks[0]), 0, -1).to(source.dtype)
    holes = t(masks) & (source < 0)
    assert holes.sum() > 0
    want, winfo = ops.exemplar_fill(base.contiguous(), holes.contiguous(), sources=t(~masks), seed=3)
    out = prepare.propagate_reference(img, masks, disp, pose, focal, refs, fill='exemplar', seed=3)
    got = out['images'].cpu().numpy()
    assert np.array_equal(bits(got), bits(want.cpu().numpy())) and np.array_equal(out['holes'].cpu().numpy(), holes.cpu().numpy())
    assert all(np.array_equal(out['info'][k], winfo[k]) for k in KEYS) and torch.equal(out['info']['nnf'], winfo['nnf'])
    assert np.array_equal(bits(got)[~masks], bits(img)[~masks])
    nnf = winfo['nnf'].cpu().numpy()
    on = nnf[..., 0] >= 0
    assert on.sum() > 0
    n_, y_, x_ = np.nonzero(on)
    assert not masks[n_, nnf[on][:, 0], nnf[on][:, 1]].any()                    # exemplars come from outside the view's mask
    # fill=True (and 'harmonic'): the composition its docstring states, bit for bit
    N, H, W = masks.shape
    planes = base.permute(0, 3, 1, 2).reshape(3 * N, H, W).contiguous()
    filled, hinfo = ops.harmonic_fill(planes, holes[:, None].expand(N, 3, H, W).reshape(3 * N, H, W).contiguous())
    hwant = torch.where(holes[..., None], filled.reshape(N, 3, H, W).permute(0, 2, 3, 1), base).cpu().numpy()
    for fill in (True, 'harmonic'):
        h = prepare.propagate_reference(img, masks, disp, pose, focal, refs, fill=fill)
        assert np.array_equal(bits(h['images'].cpu().numpy()), bits(hwant)) and np.array_equal(h['info']['iterations'], hinfo['iterations'])
    default = prepare.propagate_reference(img, masks, disp, pose, focal, refs)
    assert np.array_equal(bits(default['images'].cpu().numpy()), bits(hwant))
    none = prepare.propagate_reference(img, masks, disp, pose, focal, refs, fill='none')
    assert none['info'] is None and np.array_equal(bits(none['images'].cpu().numpy()), bits(base.cpu().numpy()))


def test_inpaint_views(cuda):
    img, _, masks, _, _ = fixture([0, 1, 5, 15])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    got = prepare.inpaint_views(img, masks, [2, 0], seed=7)
    want, info = ops.exemplar_fill(t(img[[2, 0]]), t(masks[[2, 0]]), seed=7)
    assert got.is_cuda and tuple(got.shape) == (2, 141, 252, 3) and torch.equal(got, want)
    assert info['levels'].tolist() == [3, 3] and (info['energy'] > 0).all()
    assert not torch.equal(got, t(img[[2, 0]])) and np.array_equal(bits(got.cpu().numpy())[~masks[[2, 0]]], bits(img[[2, 0]])[~masks[[2, 0]]])
    with pytest.raises(ValueError, match='no exemplar'):
        prepare.inpaint_views(img[:1], np.ones_like(masks[:1]), [0])
