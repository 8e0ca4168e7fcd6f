"""The camera restatement (tests/camera_numpy.py, the definition of csrc/camera_device.h) against first principles, on the CPU:
unproject then project brings every pixel back to itself in both precisions, and in_image is closed at the last pixel and
false for a NaN."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_numpy as C                                 # noqa: E402

H, W, FOCAL = 5, 7, 9.0
ANGLES, ORIGIN = (0.3, -0.5, 0.2), (0.4, -0.7, 1.3)
EPS32 = float(np.finfo(np.float32).eps)
# The round-trip error of a position relative to max(H, W) pixels, and of a depth relative to the depth.  fp32: measured on
# this case 0.86 eps32 and 0.19 eps32 max(H, W) -- the pose rounded to fp32 is orthonormal to eps32 only, and f / t amplifies the
# point's error into pixels -- and bounded at four times that.  fp64: 2^-40 (measured: 3e-4 of it), far above eps64 and far below
# eps32.
BOUND = {np.float32: (4 * 0.86 * EPS32, 4 * 0.19 * EPS32 * max(H, W)), np.float64: (2.0 ** -40, 2.0 ** -40)}


def round_trip(T):
    ys, xs = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    P, f = C.pose(ANGLES, ORIGIN, dtype=T), T(FOCAL)
    t = (1.5 + 0.25 * xs + 0.5 * ys).astype(T)           # a different depth at every pixel
    u, v, z = C.project(T, P, f, H, W, C.unproject(T, P, H, W, f, xs, ys, t))
    assert u.dtype == T and v.dtype == T and z.dtype == T
    wide = lambda a: a.astype(np.float64)
    e_uv = max(np.abs(wide(u) - xs).max(), np.abs(wide(v) - ys).max()) / max(H, W)
    e_z = (np.abs(wide(z) - wide(t)) / wide(t)).max()
    return float(e_uv), float(e_z)


@pytest.mark.parametrize('T', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_unproject_then_project_returns_the_pixel_and_its_depth(T):
    e_uv, e_z = round_trip(T)
    print(f'{T.__name__}: position error {e_uv / EPS32:.3g} eps32 max(H, W) pixels, depth error {e_z / EPS32:.3g} eps32 t')
    assert e_uv <= BOUND[T][0] and e_z <= BOUND[T][1]


@pytest.mark.parametrize('T', [np.float32, np.float64], ids=['fp32', 'fp64'])
def test_in_image_is_closed_at_the_last_pixel_and_false_for_nan(T):
    one, nan = T(1), T(np.nan)
    last_u, last_v = T(W - 1), T(H - 1)
    a = lambda *v: np.array(v, T)
    assert C.in_image(a(one), a(last_u), a(last_v), H, W).all() and C.in_image(a(one), a(0), a(0), H, W).all()
    assert not C.in_image(a(one), a(np.nextafter(last_u, T(np.inf))), a(0), H, W).any()
    assert not C.in_image(a(one), a(0), a(np.nextafter(last_v, T(np.inf))), H, W).any()
    assert not C.in_image(a(one, one), a(-np.nextafter(T(0), one), 0), a(0, -np.nextafter(T(0), one)), H, W).any()
    assert not C.in_image(a(0, -one), a(1, 1), a(1, 1), H, W).any()                     # z <= 0
    assert not C.in_image(a(nan, one, one), a(1, nan, 1), a(1, 1, nan), H, W).any()      # a NaN in any of the three
    # the footprint of the last pixel is the last 2 x 2 block with all the weight on its upper corner
    x0, y0, fx, fy = C.lower_footprint(a(last_u), a(last_v), H, W)
    assert (x0[0], y0[0], fx[0], fy[0]) == (W - 2, H - 2, 1, 1)
    img = np.arange(H * W, dtype=T).reshape(H, W)
    assert C.lower_blend(img, y0, x0, fy, fx)[0] == img[H - 1, W - 1]
