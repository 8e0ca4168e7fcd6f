"""Inpainted-depth preparation without a GPU: the restatement (tests/harmonic_numpy.py) against a dense solve, the argument
checks of the mvip_harmonic_* / mvip_mask_dilate2d entry points with NULL operands, the ops wrappers' refusals, the
write_llff -> load_llff._load_data round trip, keyword defaults and the tool's --help."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harmonic_cases as C                               # noqa: E402
import harmonic_numpy as R                               # noqa: E402

from mvip_nerf_amd import _lib, load_llff, ops, prepare  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL = 0, -1
P0 = None            # NULL


def raw(name, *args):
    return getattr(_lib.load(), name)(*args)


@pytest.mark.parametrize('name', C.SMALL)
def test_restatement_equals_dense_solve(name):
    v, m = C.case(name)
    U = R.unknown_set(v, m)
    sparse, singular = R.solve(v, m)
    dense = R.solve_dense(v, m)
    assert not singular and np.array_equal(sparse[~U], v[~U].astype(np.float64))
    assert np.abs(sparse - dense)[U].max() <= 1e-12
    # the equations themselves, written as loops
    H, W = v.shape
    worst = 0.0
    for y, x in zip(*np.nonzero(U)):
        nb = [(y + dy, x + dx) for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)) if 0 <= y + dy < H and 0 <= x + dx < W]
        worst = max(worst, abs(len(nb) * sparse[y, x] - sum(sparse[q] for q in nb)))
    assert worst <= 1e-12
    c32, it, ok = R.cg32(v, m)
    assert ok and it >= 1 and np.array_equal(c32[~U].view(np.int32), v[~U].view(np.int32))
    assert np.abs(c32 - sparse)[U].max() <= 1e-5
    lo, hi = v[~U].min(), v[~U].max()
    assert sparse[U].min() >= lo and sparse[U].max() <= hi                      # the maximum principle


def test_restatement_edge_cases():
    v = C.smooth(6, 9, 0)
    out, singular = R.solve(v, np.zeros(v.shape, bool))
    assert not singular and np.array_equal(out, v.astype(np.float64))
    out, singular = R.solve(v, np.ones(v.shape, bool))
    assert singular and np.array_equal(out, v.astype(np.float64))
    assert R.cg32(v, np.zeros(v.shape, bool))[1:] == (0, True) and R.cg32(v, np.ones(v.shape, bool))[1:] == (0, False)
    a = C.affine()
    m = np.zeros(a.shape, bool)
    m[10:30, 12:40] = True
    assert np.abs(R.solve_dense(a.astype(np.float32), m) - a.astype(np.float32).astype(np.float64))[~m].max() == 0
    A, b, deg, U, _ = R.system(a.astype(np.float32), m)
    assert np.abs(A @ a[U] - (A @ a[U] - b + b)).max() == 0 and np.abs(A @ a[U] - b).max() <= 1e-6   # affine is harmonic
    assert (A != A.T).nnz == 0 and set(np.unique(deg)) <= {2.0, 3.0, 4.0}
    # dilation: Chebyshev ball, clipped
    m = np.zeros((7, 9), bool)
    m[0, 0] = m[4, 5] = True
    d2 = R.dilate(m, 2)
    want = np.zeros((7, 9), bool)
    want[0:3, 0:3] = want[2:7, 3:8] = True
    assert np.array_equal(d2, want) and np.array_equal(R.dilate(m, 0), m)


def test_entry_point_argument_checks():
    for name, n in (('mvip_harmonic_tiles', 2), ('mvip_harmonic_workspace_bytes', 3), ('mvip_harmonic_setup', 9),
                    ('mvip_harmonic_init', 9), ('mvip_harmonic_iterate', 11), ('mvip_harmonic_finish', 9), ('mvip_mask_dilate2d', 6)):
        assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n
    assert raw('mvip_harmonic_tiles', 16, 64) == 1 and raw('mvip_harmonic_tiles', 17, 65) == 4
    assert raw('mvip_harmonic_tiles', 1128, 2016) == 71 * 32
    assert raw('mvip_harmonic_tiles', 0, 5) == -1 and raw('mvip_harmonic_tiles', 5, 16385) == -1
    assert raw('mvip_harmonic_workspace_bytes', 0, 5, 5) == 0 and raw('mvip_harmonic_workspace_bytes', -1, 5, 5) == -1
    assert raw('mvip_harmonic_workspace_bytes', 2, 33, 47) >= 2 * 33 * 47 * 21
    assert raw('mvip_harmonic_workspace_bytes', 1 << 40, 33, 47) == -1
    good = (3, 33, 47)
    for N, H, W in ((-1, 33, 47), (3, 0, 47), (3, 33, 0), (3, 33, 16385), (1 << 31, 33, 47)):
        assert raw('mvip_harmonic_setup', P0, P0, N, H, W, P0, P0, P0, P0) == EINVAL
        assert raw('mvip_harmonic_init', P0, N, H, W, P0, P0, P0, 1, P0) == EINVAL
        assert raw('mvip_harmonic_iterate', N, H, W, P0, P0, P0, 1, 0, 4, 1e-7, P0) == EINVAL
        assert raw('mvip_harmonic_finish', N, H, W, P0, P0, P0, 1, 1e-7, P0) == EINVAL
        assert raw('mvip_mask_dilate2d', P0, N, H, W, P0, P0) == EINVAL
    assert raw('mvip_harmonic_setup', P0, P0, 0, 0, 47, P0, P0, P0, P0) == EINVAL           # a bad shape also with no image
    # no image: MVIP_OK with NULL operands; a good shape with NULL operands: refused
    assert raw('mvip_harmonic_setup', P0, P0, 0, 33, 47, P0, P0, P0, P0) == OK
    assert raw('mvip_harmonic_init', P0, 0, 33, 47, P0, P0, P0, 1, P0) == OK
    assert raw('mvip_harmonic_iterate', 0, 33, 47, P0, P0, P0, 1, 0, 4, 1e-7, P0) == OK
    assert raw('mvip_harmonic_finish', 0, 33, 47, P0, P0, P0, 1, 1e-7, P0) == OK
    assert raw('mvip_mask_dilate2d', P0, 0, 33, 47, P0, P0) == OK
    assert raw('mvip_harmonic_setup', P0, P0, *good, P0, P0, P0, P0) == EINVAL
    assert raw('mvip_harmonic_init', P0, *good, P0, P0, P0, 1, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, 0, 4, 1e-7, P0) == EINVAL
    assert raw('mvip_harmonic_finish', *good, P0, P0, P0, 1, 1e-7, P0) == EINVAL
    assert raw('mvip_mask_dilate2d', P0, *good, P0, P0) == EINVAL
    # more active tiles than the image has (33 x 47: 3), negative counts, eps outside [0, 1)
    assert raw('mvip_harmonic_init', P0, *good, P0, P0, P0, 4, P0) == EINVAL
    assert raw('mvip_harmonic_init', P0, *good, P0, P0, P0, -1, P0) == EINVAL
    assert raw('mvip_harmonic_init', P0, *good, P0, P0, P0, 0, P0) == OK                     # no active tile: nothing launched
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 4, 0, 4, 1e-7, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, -1, 4, 1e-7, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, 0, -4, 1e-7, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, (1 << 31) - 2, 4, 1e-7, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, 0, 4, 1.0, P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, 0, 4, float('nan'), P0) == EINVAL
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 1, 0, 0, 1e-7, P0) == OK          # no iteration: nothing launched
    assert raw('mvip_harmonic_iterate', *good, P0, P0, P0, 0, 0, 4, 1e-7, P0) == OK
    assert raw('mvip_harmonic_finish', *good, P0, P0, P0, 1, -1e-7, P0) == EINVAL


def test_ops_wrappers_refuse_bad_arguments():
    v, m = torch.zeros(2, 5, 7), torch.zeros(2, 5, 7, dtype=torch.bool)
    with pytest.raises(ValueError, match='GPU'):
        ops.harmonic_fill(v, m)
    with pytest.raises(ValueError, match='GPU'):
        ops.mask_dilate2d(m, 1)
    with pytest.raises(ValueError, match='GPU'):
        ops.harmonic_fill(v.numpy(), m.numpy())
    meta = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)

    def check(fn, match):
        with pytest.raises(ValueError, match=match):
            fn()
    check(lambda: ops.harmonic_fill(meta(2, 5, 7, dtype=torch.float64), meta(2, 5, 7, dtype=torch.bool)), 'float32')
    check(lambda: ops.harmonic_fill(meta(2, 5, 7), meta(2, 5, 7, dtype=torch.uint8)), 'bool')
    check(lambda: ops.harmonic_fill(meta(5, 7), meta(5, 7, dtype=torch.bool)), r'\[N, H, W\]')
    check(lambda: ops.harmonic_fill(meta(2, 5, 7), meta(2, 5, 8, dtype=torch.bool)), 'masks')
    check(lambda: ops.harmonic_fill(meta(2, 5, 14)[:, :, ::2], meta(2, 5, 7, dtype=torch.bool)), 'contiguous')
    check(lambda: ops.harmonic_fill(meta(2, 5, 7), meta(2, 5, 7, dtype=torch.bool), eps=1.0), 'eps')
    check(lambda: ops.harmonic_fill(meta(2, 5, 7), meta(2, 5, 7, dtype=torch.bool), max_iters=-1), 'max_iters')
    check(lambda: ops.harmonic_fill(meta(2, 5, 7), meta(2, 5, 7, dtype=torch.bool), check_every=0), 'check_every')
    check(lambda: ops.mask_dilate2d(meta(2, 5, 7), 1), 'bool')
    check(lambda: ops.mask_dilate2d(meta(5, 7, dtype=torch.bool), 1), r'\[N, H, W\]')
    check(lambda: ops.mask_dilate2d(meta(2, 5, 7, dtype=torch.bool), -1), 'rounds')


def test_keyword_defaults():
    p = inspect.signature(ops.harmonic_fill).parameters
    assert (p['eps'].default, p['max_iters'].default, p['check_every'].default) == (1e-7, None, 32)
    p = inspect.signature(prepare.prepare_depths).parameters
    assert p['dilate'].default == 0 and p['allow_unconverged'].default is False and p['chunk'].default == 1 << 15
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in p.values())
    assert inspect.signature(prepare.render_disparities).parameters['chunk'].default == 1 << 15
    assert list(inspect.signature(prepare.write_llff).parameters) == ['root', 'names', 'masks', 'depths']
    with pytest.raises(ValueError, match='poses'):
        prepare.render_disparities({}, (4, 4, 1.0), np.zeros((2, 4, 4), np.float32), 1.0, 2.0)
    with pytest.raises(ValueError, match='poses'):
        prepare.prepare_depths({}, (4, 4, 1.0), np.zeros((3, 4), np.float32), np.zeros((1, 4, 4), bool), 1.0, 2.0)


def test_write_llff_round_trip(tmp_path):
    rs = np.random.RandomState(5)
    N, H, W = 3, 9, 13
    depths = rs.uniform(0.0, 1.0, (N, H, W)).astype(np.float32)
    depths[0, 0, :4] = [-0.25, 1.5, np.nan, np.inf]          # four clipped pixels
    depths[1, 2, 3], depths[1, 2, 4] = 0.0, 1.0              # the ends of the range are not
    masks = rs.rand(N, H, W) < 0.3
    names = ['20220819_104221', '20220819_104228', 'view_c']
    root = tmp_path / 'scene' / 'images_4'
    clipped = prepare.write_llff(str(root), names, torch.from_numpy(masks), torch.from_numpy(depths))
    assert clipped == 4
    assert sorted(os.listdir(root)) == ['Depth_inpainted', 'label']
    assert sorted(os.listdir(root / 'label')) == sorted(n + '.png' for n in names) == sorted(os.listdir(root / 'Depth_inpainted'))
    # the rest of a scene directory, as the loader wants it: the images and poses_bounds.npy
    os.makedirs(root / 'RGB_inpainted')
    from mvip_nerf_amd import run
    for n in names:
        run._write_png(str(root / 'RGB_inpainted' / (n + '.png')), rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
    np.save(tmp_path / 'scene' / 'poses_bounds.npy', rs.rand(N, 17))
    _, _, imgs, got_masks, got_depths, mask_indices = load_llff._load_data(str(tmp_path / 'scene'), factor=4)
    want8 = np.round(np.clip(np.where(np.isfinite(depths), depths.astype(np.float64), 0.0), 0.0, 1.0) * 255.0)
    assert want8[0, 0, :4].tolist() == [0.0, 255.0, 0.0, 0.0]
    assert got_depths.shape == (H, W, N) and np.array_equal(np.moveaxis(got_depths, -1, 0), want8 / 255.)
    assert np.array_equal(np.moveaxis(got_masks, -1, 0), masks.astype(np.float64)) and mask_indices == [0, 1, 2]
    assert np.abs(np.moveaxis(got_depths, -1, 0) - np.clip(np.nan_to_num(depths, nan=0.0, posinf=0.0), 0, 1)).max() <= 0.5 / 255 + 1e-7
    with pytest.raises(ValueError, match='names'):
        prepare.write_llff(str(root), names[:2], masks, depths)


def test_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'prepare_depths.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--fixture' in r.stdout and '--dilate' in r.stdout and '--out' in r.stdout
