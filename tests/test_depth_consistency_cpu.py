"""Cross-view depth consistency without a GPU: the restatement (tests/depth_consistency_numpy.py) on the three-camera trial
scene -- occlusions, agreement, a floater -- the argument checks of mvip_depth_consistency with NULL operands, the binding
table and the wrappers' refusals."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_consistency_numpy as R                      # noqa: E402
import warp_numpy as wn                                  # noqa: E402

from mvip_nerf_amd import _lib, ops, prepare             # noqa: E402

OK, EINVAL = 0, -1
P0 = None            # NULL


@pytest.fixture(scope='module')
def scene():
    return R.trial_scene3()


def per_camera(case, n, tol=0.05):
    """For view n and each other camera s: (agree, violated) of the two-view problem (n, s), as [H, W] arrays of 0 / 1."""
    out = {}
    for s in range(len(case['poses'])):
        if s != n:
            a, v = R.consistency(case['disp'][[n, s]], case['poses'][[n, s]], case['focal'], tol)
            out[s] = (a[0], v[0])
    return out


def test_counts_are_sums_over_the_other_cameras(scene):
    agree, violated = R.consistency(scene['disp'], scene['poses'], scene['focal'])
    assert agree.dtype == np.int32 and violated.dtype == np.int32 and agree.shape == scene['disp'].shape
    for n in range(3):
        pairs = per_camera(scene, n)
        assert np.array_equal(agree[n], sum(a for a, _ in pairs.values()))
        assert np.array_equal(violated[n], sum(v for _, v in pairs.values()))
    assert agree.max() == 2
    # a true scene: nothing is seen through, except along the box's outline, where the other view's bilinear taps mix box and wall
    assert (violated > 0).mean() < 0.02


def test_hidden_wall_pixels_get_no_evidence_and_visible_ones_agree(scene):
    H, W, f = scene['H'], scene['W'], scene['focal']
    checked_hidden = checked_seen = 0
    for n in range(3):
        pairs = per_camera(scene, n)
        for s, (a, v) in pairs.items():
            hidden = wn.hidden_from(scene['points'][n], scene['poses'][s][:, 3], **wn.TRIAL_BOX)
            assert hidden.sum() > 10                          # the box does hide wall from this camera
            assert not a[hidden].any() and not v[hidden].any()         # occluded: no agreement and no violation
            checked_hidden += int(hidden.sum())
            # what both cameras see: the point projects at least a pixel inside the other image, is not hidden, and does not
            # land within a pixel of the box's outline there (where the bilinear taps mix wall and box)
            ts, u, vv = R.project(scene['points'][n], scene['poses'][s], f, H, W)
            inside = (ts > 0) & (u >= 1) & (u <= W - 2) & (vv >= 1) & (vv <= H - 2)
            loose = wn.hidden_from(scene['points'][n], scene['poses'][s][:, 3], margin=-0.1, **wn.TRIAL_BOX)
            on_box = np.abs(scene['points'][n][..., 2] - wn.TRIAL_BOX['box_z']) < 1e-6
            bx, by = wn.TRIAL_BOX['box_x'], wn.TRIAL_BOX['box_y']
            p = scene['points'][n]
            box_interior = on_box & (p[..., 0] > bx[0] + .1) & (p[..., 0] < bx[1] - .1) & (p[..., 1] > by[0] + .1) & (p[..., 1] < by[1] - .1)
            seen = inside & ((~on_box & ~loose) | box_interior)
            assert seen.sum() > 500
            assert a[seen].all() and not v[seen].any()
            checked_seen += int(seen.sum())
    assert checked_hidden > 100 and checked_seen > 5000


def test_floater_is_violated_by_every_camera_it_lands_in_and_agreed_by_none(scene):
    case = R.with_floater(scene)
    agree, violated = R.consistency(case['disp'], case['poses'], case['focal'])
    H, W, f = case['H'], case['W'], case['focal']
    # the floater's world points: view 0's pixels at 1 / 1.5 of the wall's depth
    o, d = wn.pixel_rays(case['poses'][0], H, W, f)
    pts = o + (1.0 / case['disp'][0].astype(np.float64))[..., None] * d
    lands = np.zeros((H, W), np.int32)
    for s in (1, 2):
        ts, u, v = R.project(pts, case['poses'][s], f, H, W)
        lands += (ts > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    patch = np.zeros((H, W), bool)
    patch[R.FLOATER] = True
    assert patch.sum() == 36 and lands[patch].min() >= 1
    assert (agree[0][patch] == 0).all()
    assert np.array_equal(violated[0][patch], lands[patch])
    # outside the patch view 0 is as before
    a0, v0 = R.consistency(scene['disp'], scene['poses'], scene['focal'])
    assert np.array_equal(agree[0][~patch], a0[0][~patch]) and np.array_equal(violated[0][~patch], v0[0][~patch])
    # and the mask built from the counts drops exactly the floater among view 0's confirmed pixels
    keep = (agree >= 1) & (violated <= 0)
    assert not keep[0][patch].any() and np.array_equal(keep[0][~patch], ((a0[0] >= 1) & (v0[0] <= 0))[~patch])


def test_invalid_pixels_are_neither_targets_nor_witnesses(scene):
    d = scene['disp'].copy()
    d[1, 10:20, 10:30] = (np.nan, np.inf, 0.0, -1.0, np.nan) * 4
    agree, violated = R.consistency(d, scene['poses'], scene['focal'])
    assert not agree[1, 10:20, 10:30].any() and not violated[1, 10:20, 10:30].any()
    m = np.ones(d.shape, bool)
    m[1, 10:20, 10:30] = False
    a2, v2 = R.consistency(scene['disp'], scene['poses'], scene['focal'], masks=m)
    assert np.array_equal(agree, a2) and np.array_equal(violated, v2)          # a masked pixel is a zeroed pixel
    a0, _ = R.consistency(scene['disp'], scene['poses'], scene['focal'])
    assert (a2 <= a0).all() and (a2 < a0).any()              # the other views lost a witness: the four-tap rule


def test_few_views():
    c = R.trial_scene3()
    for V in (0, 1):
        a, v = R.consistency(c['disp'][:V], c['poses'][:V], c['focal'])
        assert a.shape == (V, c['H'], c['W']) and not a.any() and not v.any()


def test_entry_point_argument_checks():
    name = 'mvip_depth_consistency'
    assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == 10 and _lib.ABI_VERSION == 5
    raw = lambda V, H, W, focal, tol: getattr(_lib.load(), name)(P0, P0, V, H, W, focal, tol, P0, P0, P0)
    for V, H, W in ((-1, 33, 47), (3, 1, 47), (3, 33, 1), (3, 0, 0), (3, 16385, 47), (3, 33, 16385), (2 ** 31 - 1, 33, 47), (0, 1, 47)):
        assert raw(V, H, W, 60.0, 0.05) == EINVAL, (V, H, W)
    for focal, tol in ((0.0, 0.05), (-1.0, 0.05), (float('nan'), 0.05), (float('inf'), 0.05), (60.0, 0.0), (60.0, -0.05),
                       (60.0, float('nan')), (60.0, float('inf'))):
        assert raw(3, 33, 47, focal, tol) == EINVAL, (focal, tol)
        assert raw(0, 33, 47, focal, tol) == EINVAL, (focal, tol)     # a bad parameter also with no view
    assert raw(0, 33, 47, 60.0, 0.05) == OK and raw(0, 2, 2, 60.0, 0.05) == OK      # no view: nothing launched
    assert raw(3, 33, 47, 60.0, 0.05) == EINVAL and raw(1, 33, 47, 60.0, 0.05) == EINVAL      # NULL operands


def test_wrappers_refuse_bad_arguments():
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    d, p = z(3, 8, 9), z(3, 3, 4)
    for args, kw in (((d.double(), p, 60.0), {}), ((d[0], p, 60.0), {}), ((d, p[:2], 60.0), {}), ((d, z(3, 4, 4), 60.0), {}),
                     ((z(3, 1, 9), p, 60.0), {}), ((d, p, 0.0), {}), ((d, p, float('nan')), {}), ((d, p, 60.0), {'tol': 0.0}),
                     ((d, p, 60.0), {'tol': float('inf')}), ((d, p, 60.0), {'masks': z(3, 8, 9)}),
                     ((d, p, 60.0), {'masks': z(3, 8, 8, dtype=torch.bool)}), ((d.numpy(), p, 60.0), {})):
        with pytest.raises(ValueError, match='depth_consistency'):
            ops.depth_consistency(*args, **kw)
    with pytest.raises(ValueError, match='no CPU fallback'):
        ops.depth_consistency(d, p, 60.0)
    with pytest.raises(ValueError, match='min_agree'):
        prepare.consistency_mask(d, p, 60.0, min_agree=-1)
    with pytest.raises(ValueError, match='max_violated'):
        prepare.consistency_mask(d, p, 60.0, max_violated=-1)
    sig = {k: v.default for k, v in inspect.signature(ops.depth_consistency).parameters.items()}
    assert sig['masks'] is None and sig['tol'] == 0.05
    sig = {k: v.default for k, v in inspect.signature(prepare.consistency_mask).parameters.items()}
    assert (sig['tol'], sig['min_agree'], sig['max_violated']) == (0.05, 1, 0)
