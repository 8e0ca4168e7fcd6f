"""The guided-fill cases shared by tests/test_poisson.py (GPU) and tests/test_poisson_cpu.py: 37 x 70 images (the tile of
csrc/harmonic.hip is 64 x 16: one tile edge in x and two in y lie inside), a smooth guide with a little noise, values = the
guide plus a constant outside the mask, labels over the mask dilated by one pixel."""
import numpy as np

import harmonic_cases as C
import harmonic_numpy as R

H, W = 37, 70
OFFSET = np.float32(0.125)
STEP = np.float32(0.3)             # what the two-label case raises the guide by for x >= SPLIT
SPLIT = 40


def guide():
    return C.smooth(H, W, 21)


def disc():
    return C.disc(H, W, 18, 40, 14)


def ring_labels(m, label=0):
    """int32: `label` on the mask dilated by one pixel, -1 elsewhere."""
    return np.where(R.dilate(m, 1), label, -1).astype(np.int32)


def case(name):
    """(v fp32, m bool, g fp32, l int32), each [H, W].  Outside the mask v = guide() + OFFSET."""
    g = guide()
    v = (g + OFFSET).astype(np.float32)
    m = disc()
    l = ring_labels(m)
    if name == 'offset':
        pass
    elif name in ('step_one_label', 'step_two_labels'):      # the guide of two sources at different levels
        g = g.copy()
        g[:, SPLIT:] += STEP
        if name == 'step_two_labels':
            l = np.where(l >= 0, (np.arange(W)[None, :] >= SPLIT).astype(np.int32), l).astype(np.int32)
    elif name == 'two_borders':                               # degrees 2 and 3
        m = np.zeros((H, W), bool)
        m[0:12, 0:20] = True
        l = ring_labels(m)
    elif name == 'tile_edges':                                # guided edges across x = 64, y = 16 and y = 32
        m = np.zeros((H, W), bool)
        m[10:36, 50:69] = True
        l = ring_labels(m)
    elif name == 'guide_nonfinite':                           # one pixel inside the mask without a guide
        g = g.copy()
        g[20, 38] = np.nan
    elif name == 'value_nonfinite':                           # a pixel of the ring becomes an unknown; it keeps its label
        v[18, 26] = np.inf
        assert not m[18, 26] and m[18, 27]
    elif name == 'ring_half_unlabelled':                      # the ring carries no source on the left side
        l = np.where(~m & (np.arange(W)[None, :] < SPLIT), -1, l).astype(np.int32)
    else:
        raise KeyError(name)
    return v, m, g, l


SOLVED = ('offset', 'step_two_labels', 'two_borders', 'tile_edges', 'guide_nonfinite', 'value_nonfinite', 'ring_half_unlabelled')


def padded(name):
    """A case of harmonic_cases that fits into H x W, pasted into the top-left corner of a smooth image."""
    v0, m0 = C.case(name)
    v, m = C.smooth(H, W, 31), np.zeros((H, W), bool)
    v[:v0.shape[0], :v0.shape[1]], m[:m0.shape[0], :m0.shape[1]] = v0, m0
    return v, m


def unguided_masks():
    """name -> (v, m): the masks of harmonic_cases that fit H x W, and a disc across the tile edges x = 64, y = 16, y = 32."""
    out = {n: padded(n) for n in ('one_pixel', 'corners', 'l_top', 'l_top_nonfinite')}
    out['disc_over_tile_edges'] = (C.smooth(H, W, 32), C.disc(H, W, 24, 60, 10))
    return out
