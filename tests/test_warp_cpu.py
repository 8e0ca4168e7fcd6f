"""Reference-view propagation without a GPU: the restatement (tests/warp_numpy.py) against per-pixel Python loops, the figures
it gives on the dataset's rasters (tests/golden/scene1_small.npz), the trial scene's occlusions, the argument checks of
mvip_warp_views with NULL operands, the refusals of ops.warp_views and prepare.propagate_reference, the write_images round
trip and the tool's --help."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_numpy as R                                   # noqa: E402

from mvip_nerf_amd import _lib, load_llff, ops, prepare  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
OK, EINVAL = 0, -1
P0 = None            # NULL


def loops(tgt_disp, tgt_pose, tgt_mask, src_rgb, src_disp, src_pose, focal, order, tol):
    """The definition of the issue, one pixel at a time in Python floats (fp64), written from the formulas and not from
    warp_numpy.warp: matrices as nested lists, the bilinear read as an explicit four-tap sum."""
    N, H, W = tgt_disp.shape
    S = src_disp.shape[0]
    rgb, index, resid = np.zeros((N, H, W, 3)), np.full((N, H, W), -1, np.int32), np.zeros((N, H, W))
    focal, tol = float(np.float32(focal)), float(np.float32(tol))
    for n in range(N):
        Rn = [[float(tgt_pose[n, r, c]) for c in range(3)] for r in range(3)]
        on = [float(tgt_pose[n, r, 3]) for r in range(3)]
        for y in range(H):
            for x in range(W):
                d = float(tgt_disp[n, y, x])
                if not tgt_mask[n, y, x] or not math.isfinite(d) or not d > 0:
                    continue
                t = 1.0 / d
                pc = [t * (x - W / 2) / focal, -t * (y - H / 2) / focal, -t]
                pw = [sum(Rn[r][c] * pc[c] for c in range(3)) + on[r] for r in range(3)]
                for k in range(S):
                    s = int(order[n, k])
                    if not 0 <= s < S:
                        continue
                    dl = [pw[r] - float(src_pose[s, r, 3]) for r in range(3)]
                    q = [sum(float(src_pose[s, r, c]) * dl[r] for r in range(3)) for c in range(3)]      # R^T dl
                    ts = -q[2]
                    if not ts > 0:
                        continue
                    u, v = focal * q[0] / ts + W / 2, -(focal * q[1]) / ts + H / 2
                    if not (0 <= u <= W - 1 and 0 <= v <= H - 1):
                        continue
                    x0, y0 = min(math.floor(u), W - 2), min(math.floor(v), H - 2)
                    fx, fy = u - x0, v - y0
                    taps = ((y0, x0, (1 - fx) * (1 - fy)), (y0, x0 + 1, fx * (1 - fy)), (y0 + 1, x0, (1 - fx) * fy), (y0 + 1, x0 + 1, fx * fy))
                    ds = sum(float(src_disp[s, a, b]) * w for a, b, w in taps)
                    col = [sum(float(src_rgb[s, a, b, c]) * w for a, b, w in taps) for c in range(3)]
                    e = ts * ds - 1.0
                    if math.isfinite(ds) and ds > 0 and abs(e) <= tol and all(math.isfinite(c) for c in col):
                        rgb[n, y, x], index[n, y, x], resid[n, y, x] = col, s, e
                        break
    return rgb, index, resid


def small_case():
    """6 x 8, two targets, three sources around a tilted plane with a step in it; an order row with an entry out of range;
    unmasked pixels, a NaN, a zero and a negative target disparity, a NaN source colour and a NaN source disparity."""
    H, W, f = 6, 8, 7.0
    rs = np.random.RandomState(3)
    poses = [R.pose((0.02 * i, -0.03 * i, 0.01), (0.12 * i - 0.2, 0.05 * i, 0.02 * i)) for i in range(5)]
    disp = lambda p: np.where(np.mgrid[0:H, 0:W][1] < 5, R.plane_disparity(p, H, W, f, (0.1, 0.05, 1.0), -3.0),
                              R.plane_disparity(p, H, W, f, (0.0, 0.0, 1.0), -2.0)).astype(np.float32)
    tgt_pose, src_pose = np.stack(poses[:2]), np.stack(poses[2:])
    tgt_disp, src_disp = np.stack([disp(p) for p in tgt_pose]), np.stack([disp(p) for p in src_pose])
    src_rgb = rs.rand(3, H, W, 3).astype(np.float32)
    mask = rs.rand(2, H, W) < 0.85
    tgt_disp[0, 1, 1], tgt_disp[0, 2, 2], tgt_disp[1, 3, 3] = np.nan, 0.0, -0.4
    src_rgb[0, 2, 3, 1], src_disp[1, 4, 4] = np.nan, np.nan
    order = np.array([[2, 7, 0], [1, -1, 2]], np.int32)
    return (tgt_disp, tgt_pose, mask, src_rgb, src_disp, src_pose, f), order


def test_restatement_equals_per_pixel_loops():
    args, order = small_case()
    for tol in (0.05, 0.5):
        want = loops(*args, order, tol)
        got = R.warp(*args, order=order, tol=tol)
        assert np.array_equal(got[1], want[1])
        assert (want[1] >= 0).sum() >= 20 and (want[1] < 0).sum() >= 20 and len(np.unique(want[1])) >= 3
        assert np.abs(got[0] - want[0]).max() <= 1e-13 and np.abs(got[2] - want[2]).max() <= 1e-13
        r32, i32, e32 = R.warp(*args, order=order, tol=tol, dtype=np.float32)
        assert r32.dtype == np.float32 and e32.dtype == np.float32
        same = i32 == want[1]
        assert same.mean() >= 0.95 and np.abs(r32 - want[0])[same].max() <= 1e-4 and np.abs(e32 - want[2])[same].max() <= 1e-4
    # nothing taken: 0 / -1 / 0, also for S = 0 and for an empty mask
    a = list(args)
    none = R.warp(a[0], a[1], np.zeros_like(a[2]), *a[3:], order=order)
    assert not none[0].any() and (none[1] == -1).all() and not none[2].any()
    none = R.warp(a[0], a[1], a[2], a[3][:0], a[4][:0], a[5][:0], a[6])
    assert not none[0].any() and (none[1] == -1).all() and not none[2].any()


def test_identity_warp_returns_the_source_and_excludes_its_border():
    c = R.homography_case()
    full = np.ones_like(c['tgt_mask'])
    y = R.yardstick(c['src_disp'], c['src_pose'], full, c['src_rgb'], c['src_disp'], c['src_pose'], c['focal'])
    ring = np.ones(full.shape, bool)
    ring[:, 1:-1, 1:-1] = False
    assert (y['index'][~ring] == 0).all() and np.abs(y['rgb'] - c['src_rgb'])[~ring].max() <= 1e-6 and np.abs(y['resid']).max() <= 1e-6
    assert np.array_equal(y['excluded'], ring)              # u = 0, u = W-1, v = 0, v = H-1 sit on the threshold


def test_trial_scene_occlusions():
    c = R.trial_scene()
    y = R.yardstick(*R.args_of(c))
    valid = y['index'][0] >= 0
    hidden = R.hidden_from(c['tgt_points'], c['src_pose'][0][:, 3], **R.TRIAL_BOX)
    print(f'trial scene: valid {valid.mean():.4f}, hidden {int(hidden.sum())}, excluded {int(y["excluded"].sum())}, fp32 run: index '
          f'differs on {y["index32_differs"]}, e32 rgb {y["e32_rgb"]:.2e} resid {y["e32_resid"]:.2e}')
    assert abs(valid.mean() - 0.87) < 0.005
    assert hidden.sum() >= 40 and not (hidden & valid).any()
    assert y['excluded'].sum() == 0 and y['index32_differs'] == 0
    assert y['e32_rgb'] <= 1e-5 and y['e32_resid'] <= 1e-5
    # what is taken is the source's image at the projected point: against the smooth part of the image the error is the noise's
    assert np.abs(y['resid'][0][valid]).max() <= 0.05


def fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    img = z['images'].astype(np.float32) / np.float32(255.)
    disp = z['depths'].astype(np.float32) / np.float32(255.)
    P = z['poses']
    H, W = img.shape[1:3]
    return img, disp, z['masks'].astype(bool), np.ascontiguousarray(P[:, :, :4]), float(P[0, 2, 4]) * W / float(P[0, 1, 4])


def test_fixture_table():
    """The figures of DESIGN.md section 15: the dataset's own 8-bit disparity rasters and poses, view 0 the only source."""
    img, disp, masks, pose, focal = fixture()
    N, H, W = disp.shape
    rms = lambda a, b, sel: float(np.sqrt(((a[sel].astype(np.float64) - b[sel]) ** 2).mean()))
    table = {1: (0.986, 0.063, 0.035, 0.180), 5: (1.000, 0.056, 0.034, 0.210), 15: (0.985, 0.081, 0.044, 0.239), 29: (0.983, 0.108, 0.060, 0.270)}
    views = sorted(table)
    for tol, lo, hi in ((0.05, None, None), (0.02, 0.76, 0.92)):
        rgb, index, _ = R.warp(disp[views], pose[views], np.ones((len(views), H, W), bool), img[:1], disp[:1], pose[:1], focal, tol=tol)
        for i, n in enumerate(views):
            valid, m = index[i] >= 0, masks[n]
            cover = float((valid & m).sum()) / float(m.sum())
            row = (cover, rms(rgb[i], img[n], valid & m), rms(rgb[i], img[n], valid), rms(img[0], img[n], np.ones_like(m)))
            print(f'tol {tol} view {n}: ' + ' '.join(f'{v:.4f}' for v in row))
            if tol == 0.05:
                assert all(abs(got - want) <= 0.5e-3 + 1e-9 for got, want in zip(row, table[n])), (n, row)
                assert row[2] <= 0.5 * row[3] and row[2] <= 0.5 * rms(img[0], img[n], valid)
            else:
                assert lo - 0.005 <= cover <= hi + 0.005


def test_entry_point_argument_checks():
    name = 'mvip_warp_views'
    assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == 17 and _lib.ABI_VERSION == 5
    raw = lambda N, H, W, S, focal, tol: getattr(_lib.load(), name)(P0, P0, P0, N, H, W, P0, P0, P0, S, P0, focal, tol, P0, P0, P0, P0)
    for N, H, W, S in ((-1, 33, 47, 1), (3, 1, 47, 1), (3, 33, 1, 1), (3, 0, 0, 1), (3, 33, 47, -1), (3, 16385, 47, 1), (1 << 31, 33, 47, 1)):
        assert raw(N, H, W, S, 60.0, 0.05) == EINVAL, (N, H, W, S)
    for focal, tol in ((0.0, 0.05), (-1.0, 0.05), (float('nan'), 0.05), (float('inf'), 0.05), (60.0, 0.0), (60.0, -0.05),
                       (60.0, float('nan')), (60.0, float('inf'))):
        assert raw(3, 33, 47, 1, focal, tol) == EINVAL, (focal, tol)
        assert raw(0, 33, 47, 1, focal, tol) == EINVAL, (focal, tol)     # a bad parameter also with no target
    assert raw(0, 1, 47, 1, 60.0, 0.05) == EINVAL                        # a bad shape also with no target
    assert raw(0, 33, 47, 1, 60.0, 0.05) == OK and raw(0, 2, 2, 0, 60.0, 0.05) == OK      # no target: nothing launched
    assert raw(3, 33, 47, 1, 60.0, 0.05) == EINVAL and raw(3, 33, 47, 0, 60.0, 0.05) == EINVAL   # NULL operands


def test_wrappers_refuse_bad_arguments(tmp_path):
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    good = lambda: dict(tgt_disp=z(2, 5, 7), tgt_pose=z(2, 3, 4), tgt_mask=z(2, 5, 7, dtype=torch.bool), src_rgb=z(3, 5, 7, 3),
                        src_disp=z(3, 5, 7), src_pose=z(3, 3, 4), focal=9.0)

    def check(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.warp_views(**dict(good(), **kw))
    check('GPU')                                                          # CPU tensors
    check('GPU', tgt_disp=np.zeros((2, 5, 7), np.float32))
    check('float32', tgt_disp=z(2, 5, 7, dtype=torch.float64))
    check('bool', tgt_mask=z(2, 5, 7, dtype=torch.uint8))
    check(r'\[N, H, W\]', src_disp=z(5, 7))
    check(r'\[N, 3, 4\]', tgt_pose=z(2, 3, 5))
    check(r'\[N, 3, 4\]', src_pose=z(3, 4, 4))
    check('float32', src_pose=z(3, 3, 4, dtype=torch.float64))
    check('src_rgb', src_rgb=z(3, 5, 7))
    check('src_rgb', src_rgb=z(3, 5, 7, 3, dtype=torch.float16))
    check('tgt_mask', tgt_mask=z(2, 5, 8, dtype=torch.bool))
    check('tgt_pose', tgt_pose=z(3, 3, 4))
    check('src_disp', src_disp=z(3, 5, 8))
    check('src_rgb', src_rgb=z(2, 5, 7, 3))
    check('src_pose', src_pose=z(2, 3, 4))
    check('2 x 2', tgt_disp=z(2, 1, 7), tgt_mask=z(2, 1, 7, dtype=torch.bool), src_disp=z(3, 1, 7), src_rgb=z(3, 1, 7, 3))
    check('focal', focal=0.0)
    check('focal', focal=float('nan'))
    check('tol', tol=-0.05)
    check('order', order=z(2, 3, dtype=torch.int64))
    check('order', order=z(3, 2, dtype=torch.int32))
    check('order', order=[[0, 1, 2], [0, 1, 2]])
    p = inspect.signature(ops.warp_views).parameters
    assert list(p) == ['tgt_disp', 'tgt_pose', 'tgt_mask', 'src_rgb', 'src_disp', 'src_pose', 'focal', 'order', 'tol']
    assert p['order'].default is None and p['tol'].default == 0.05
    # bytes from shapes (the bench tool's): 25 per target pixel, 16 per source pixel
    from tools import warp_bench
    assert warp_bench.hbm_bytes(60, 564, 1008, 3) == 60 * 564 * 1008 * 25 + 3 * 564 * 1008 * 16

    p = inspect.signature(prepare.propagate_reference).parameters
    assert list(p)[:9] == ['images', 'masks', 'disparities', 'poses', 'focal', 'ref_views', 'ref_images', 'tol', 'fill']
    assert p['ref_images'].default is None and p['tol'].default == 0.05 and p['fill'].default is True
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in p.values())
    img, m, d, poses = np.zeros((4, 5, 7, 3), np.float32), np.zeros((4, 5, 7), bool), np.ones((4, 5, 7), np.float32), np.zeros((4, 3, 4), np.float32)

    def refuse(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            prepare.propagate_reference(*a, **kw)
    refuse('ref_views', img, m, d, poses, 9.0, [])
    refuse('ref_views', img, m, d, poses, 9.0, [4])
    refuse('ref_views', img, m, d, poses, 9.0, [1, 1])
    refuse('images', img[..., 0], m, d, poses, 9.0, [0])
    refuse('masks', img, m[:3], d, poses, 9.0, [0])
    refuse('disparities', img, m, d[:, :4], poses, 9.0, [0])
    refuse('poses', img, m, d, np.zeros((4, 3, 5), np.float32), 9.0, [0])
    refuse('poses', img, m, d, poses[:3], 9.0, [0])
    refuse('ref_images', img, m, d, poses, 9.0, [0, 2], ref_images=img[:1])
    # the order of the references: by camera-centre distance, ties by position in ref_views
    poses[:, 0, 3] = [0.0, 1.0, 2.0, 3.0]
    assert prepare.reference_order(poses, [3, 1]).tolist() == [[1, 0], [1, 0], [0, 1], [0, 1]]      # view 2: a tie


def test_write_images_round_trip(tmp_path):
    rs = np.random.RandomState(6)
    N, H, W = 3, 9, 13
    img = rs.uniform(0.0, 1.0, (N, H, W, 3)).astype(np.float32)
    img[0, 0, :4, 0] = [-0.25, 1.5, np.nan, np.inf]          # four clipped values
    img[1, 2, 3, 1], img[1, 2, 4, 2] = 0.0, 1.0              # the ends of the range are not
    names = ['20220819_104221', '20220819_104228', 'view_c']
    root = tmp_path / 'scene' / 'images_4'
    assert prepare.write_images(str(root), names, torch.from_numpy(img)) == 4
    assert os.listdir(root) == ['RGB_inpainted'] and sorted(os.listdir(root / 'RGB_inpainted')) == sorted(n + '.png' for n in names)
    want = np.round(np.clip(np.where(np.isfinite(img), img.astype(np.float64), 0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert want[0, 0, :4, 0].tolist() == [0, 255, 0, 0]
    for i, n in enumerate(names):
        got = load_llff._imread(str(root / 'RGB_inpainted' / (n + '.png')))
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want[i])
    with pytest.raises(ValueError, match='names'):
        prepare.write_images(str(root), names[:2], img)
    assert list(inspect.signature(prepare.write_images).parameters) == ['root', 'names', 'images']
    assert list(inspect.signature(prepare.write_llff).parameters) == ['root', 'names', 'masks', 'depths']


def test_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'propagate_reference.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for opt in ('--fixture', '--datadir', '--factor', '--ref-views', '--ref-image', '--tol', '--depths', '--checkpoint', '--out'):
        assert opt in r.stdout, opt
