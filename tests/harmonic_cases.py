"""The harmonic-fill cases shared by tests/test_prepare.py (GPU) and tests/test_prepare_cpu.py: smooth fp32 images with a
little noise and the masks that exercise every path of csrc/harmonic.hip (one unknown, degree-2 corners, a hole on the
border, a band that touches both side borders, two holes in one image with a known pixel inside one, one wide hole of
several hundred tiles, non-finite known pixels)."""
import numpy as np


def smooth(H, W, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    v = 0.3 + 0.1 * np.sin(x / 9.0) + 0.08 * np.cos(y / 7.0) + 0.0005 * (x - y) + 0.002 * rs.randn(H, W)
    return v.astype(np.float32)


def disc(H, W, cy, cx, r):
    y, x = np.mgrid[0:H, 0:W]
    return (y - cy) ** 2 + (x - cx) ** 2 < r * r


def l_shape():
    m = np.zeros((33, 47), bool)
    m[0:20, 10:18] = True
    m[14:20, 10:35] = True
    return m


def case(name):
    """(v fp32 [H, W], m bool [H, W])"""
    if name == 'one_pixel':
        m = np.zeros((8, 8), bool)
        m[3, 4] = True
        return smooth(8, 8, 1), m
    if name == 'corners':
        m = np.zeros((8, 8), bool)
        m[0, 0] = m[0, 7] = m[7, 7] = True
        return smooth(8, 8, 2), m
    if name == 'l_top':
        return smooth(33, 47, 3), l_shape()
    if name == 'band':
        m = np.zeros((64, 64), bool)
        m[24:40, :] = True
        return smooth(64, 64, 4), m
    if name == 'disc_and_box':
        m = disc(96, 128, 48, 50, 30)
        m[48, 50] = False
        m[10:25, 100:120] = True
        return smooth(96, 128, 5), m
    if name == 'disc200':
        return smooth(512, 512, 6), disc(512, 512, 256, 256, 200)
    if name == 'l_top_nonfinite':
        v = smooth(33, 47, 3)
        v[25, 30] = np.nan
        v[13, 18] = np.inf                      # a known neighbour of the hole: becomes an unknown, the hole grows
        return v, l_shape()
    raise KeyError(name)


SMALL = ('one_pixel', 'corners', 'l_top', 'band', 'disc_and_box', 'l_top_nonfinite')
ALL = ('one_pixel', 'corners', 'l_top', 'band', 'disc_and_box', 'disc200', 'l_top_nonfinite')


def affine(H=40, W=50):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return 0.2 + 0.003 * x - 0.002 * y
