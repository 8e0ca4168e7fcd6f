"""numpy restatement of regions (mvip_nerf_amd/region.py, csrc/region.hip), written from the conventions alone; the grid
is occupancy's, so cell_of / pack / unpack / dilate come from tests/occupancy_numpy.py.

inside(p) = in the box AND bit set (occupancy's keep(p) is "outside the box OR bit set").
mark: the cells that hold a point, OR-ed into the cells already set.  accumulate: per ray, the sum in fp64 of the fp32
weights of the samples whose point is inside (a select: a weight outside the region is not read into the sum).
carve: the complement cells (as words: tail bits zero).  default_box: per axis e = max - min over the finite points,
h = e / (cells - 2 (dilate + 1)), bmin = min - (dilate + 1) h, bmax = max + (dilate + 1) h.
"""
import numpy as np

import occupancy_numpy as R


def inside(pts, bmin, bmax, cells, reg):
    """bool [P]: in the box and in a cell of the region (reg: bool [cx, cy, cz])."""
    in_box, l = R.cell_of(pts, bmin, bmax, cells)
    return in_box & np.asarray(reg, bool).reshape(-1)[l]


def mark(pts, bmin, bmax, cells, reg=None):
    """bool [cx, cy, cz]: reg (or nothing) plus the cells that hold a point of pts [P, 3]."""
    out = np.zeros(cells, bool) if reg is None else np.array(reg, bool)
    in_box, l = R.cell_of(pts, bmin, bmax, cells)
    out.reshape(-1)[l[in_box]] = True
    return out


def accumulate(pts, weights, bmin, bmax, cells, reg):
    """float64 [B]: pts [B, S, 3] fp32 (the sample points as the pass under test formed them), weights [B, S] fp32."""
    B, S = weights.shape
    m = inside(np.asarray(pts, np.float32).reshape(-1, 3), bmin, bmax, cells, reg).reshape(B, S)
    return np.where(m, np.asarray(weights, np.float32).astype(np.float64), 0.0).sum(1), m


def carve(reg):
    """The complement cells, and their words."""
    c = ~np.asarray(reg, bool)
    return c, R.pack(c)


def default_box(pts, cells, dilate):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(1)]
    lo, hi = pts.min(0), pts.max(0)
    pad = dilate + 1
    h = (hi - lo) / (np.asarray(cells, np.float64) - 2 * pad)
    return (lo - pad * h).astype(np.float32), (hi + pad * h).astype(np.float32)
