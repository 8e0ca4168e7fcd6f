"""Occupancy grids for empty-space skipping in no-grad renders (beyond the reference: MVIP-NeRF evaluates every sample).

Rendering with a grid (`render_kwargs['occupancy'] = grid`, run.render_rays) means: the render the ordinary chain would
produce if the network's raw output were replaced by zeros (rgb_raw = 0, sigma = 0) at every sample whose point lies in a
cell the grid marks empty -- and the network is never evaluated at those samples.  A sample with sigma = 0 has alpha = 0 and
weight 0, so on a grid that is conservative the render equals the ordinary one; whether a grid is conservative is the
builder's business (from_density / from_model: threshold, samples_per_cell, dilate).

Conventions (shared with csrc/occupancy.hip and the test restatement tests/occupancy_numpy.py): box [bmin, bmax], cells =
(cx, cy, cz), each 1..512; inv = cells / (bmax - bmin), formed once in fp64 and rounded to fp32.  Cell of a point p, per
axis in fp32: f = floorf((p - bmin) * inv); p is inside the box iff 0 <= f < c on all three axes (a NaN or infinite
coordinate fails the comparison: outside).  Linear cell l = (ix * cy + iy) * cz + iz (z fastest, like mesh.py), bit l & 31
of int32 word l >> 5, unused tail bits zero.  keep(p) = outside the box, or bit set: points outside the box are always
evaluated.  There is no CPU path: the words live on the device.
"""
import math

import numpy as np
import torch

from . import mesh, ops

MAX_CELLS_PER_AXIS = 512
MAX_SAMPLES_PER_CELL = 8
# from_model's default: the largest threshold of tools/render_occupancy_ab.py's sweep that keeps the held-out PSNR of the
# 1,500-iteration scene-1 field within 0.05 dB of the ordinary render (profiles/occupancy_ab.json)
DEFAULT_THRESHOLD = 5.0
FORMAT_VERSION = 1


def _cells(cells):
    c = (int(cells),) * 3 if np.isscalar(cells) else tuple(int(n) for n in cells)
    if len(c) != 3 or not all(1 <= n <= MAX_CELLS_PER_AXIS for n in c):
        raise ValueError(f'cells {c}: three axes of 1..{MAX_CELLS_PER_AXIS} cells each')
    return c


def _threshold(threshold):
    threshold = float(threshold)
    if not (threshold >= 0 and math.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
    return threshold


def _count(name, v, lo, hi):
    if int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f'{name} must be an integer in {lo}..{hi}, got {v!r}')
    return int(v)


def cell_inverse(bmin, bmax, cells):
    """inv [3] fp32 = cells / (bmax - bmin), the quotient formed in fp64 and rounded once."""
    return (np.asarray(cells, np.float64) / (bmax.astype(np.float64) - bmin.astype(np.float64))).astype(np.float32)


class OccupancyGrid:
    """One bit per cell of an axis-aligned box.  `words`: int32 [(cx cy cz + 31) // 32] on the device the grid is used on
    (a numpy array or CPU tensor is accepted where no kernel is called: save / load / occupied_fraction)."""

    def __init__(self, bmin, bmax, cells, words):
        self.bmin, self.bmax = mesh._bounds(bmin, bmax)
        self.cells = _cells(cells)
        self.inv = cell_inverse(self.bmin, self.bmax, self.cells)
        if not (np.all(np.isfinite(self.inv)) and np.all(self.inv > 0)):
            raise ValueError('the box is too thin or too large: cells / (bmax - bmin) is not a finite fp32 number')
        if not torch.is_tensor(words):
            words = torch.from_numpy(np.ascontiguousarray(np.asarray(words)))
        n = ops.occupancy_words(self.cells)
        if words.dtype != torch.int32 or tuple(words.shape) != (n,):
            raise ValueError(f'words must be int32 [{n}] for cells {self.cells}, got {words.dtype} {tuple(words.shape)}')
        self.words = words.contiguous()
        self.reset_stats()

    # -- bookkeeping of the renders that used this grid (run.render_rays adds to it) ----------------------------------
    def reset_stats(self):
        """stats: samples / kept samples per pass and the number of network launches, summed over the render_rays calls
        since the last reset."""
        self.stats = {'samples_coarse': 0, 'kept_coarse': 0, 'samples_fine': 0, 'kept_fine': 0, 'network_launches': 0}

    @property
    def device(self):
        return self.words.device

    @property
    def n_cells(self):
        return self.cells[0] * self.cells[1] * self.cells[2]

    def box(self):
        """(bmin, inv) as the six floats the kernels take."""
        return [float(v) for v in self.bmin] + [float(v) for v in self.inv]

    def to(self, device):
        return OccupancyGrid(self.bmin, self.bmax, self.cells, self.words.to(device))

    def occupied_fraction(self):
        w = self.words.detach().cpu().numpy().view(np.uint32)
        return float(np.unpackbits(w.view(np.uint8)).sum()) / self.n_cells

    def lookup(self, pts):
        """keep(p) of pts [..., 3] (device): bool [P], True = outside the box or in an occupied cell."""
        if not torch.is_tensor(pts) or pts.shape[-1] != 3:
            raise ValueError('pts must be a [..., 3] torch tensor on the GPU')
        if pts.device != self.words.device:
            raise ValueError(f'pts on {pts.device}, the grid on {self.words.device}')
        return ops.occupancy_lookup(pts, self.box(), self.cells, self.words).bool()

    def save(self, path):
        """An .npz of the words and the five small arrays (bmin, bmax, cells, inv, version)."""
        np.savez(path, words=self.words.detach().cpu().numpy(), bmin=self.bmin, bmax=self.bmax,
                 cells=np.asarray(self.cells, np.int32), inv=self.inv, version=np.asarray([FORMAT_VERSION], np.int32))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as d:
            missing = [k for k in ('words', 'bmin', 'bmax', 'cells', 'inv', 'version') if k not in d.files]
            if missing:
                raise ValueError(f'{path}: not an occupancy grid file (missing {missing})')
            if int(d['version'][0]) != FORMAT_VERSION:
                raise ValueError(f'{path}: format version {int(d["version"][0])}, expected {FORMAT_VERSION}')
            words, bmin, bmax, cells, inv = d['words'], d['bmin'], d['bmax'], d['cells'], d['inv']
        g = cls(bmin, bmax, tuple(int(c) for c in cells), torch.from_numpy(words.astype(np.int32, copy=False)))
        if not np.array_equal(g.inv, inv.astype(np.float32)):
            raise ValueError(f'{path}: stored cell scale {inv.tolist()} differs from the one its box gives {g.inv.tolist()}')
        return g if device is None else g.to(device)

    @classmethod
    def from_density(cls, sigma, bmin, bmax, threshold, samples_per_cell=1, dilate=1):
        """sigma: device tensor [cx k + 1, cy k + 1, cz k + 1] (k = samples_per_cell) in mesh.density_grid's point
        convention; cell (i, j, l) owns points i k .. (i + 1) k inclusive on each axis and is occupied iff any of them has
        !(sigma <= threshold) (NaN counts as occupied).  Then `dilate` rounds of: occupied iff any cell at Chebyshev
        distance <= 1 is occupied (clipped at the faces)."""
        if not torch.is_tensor(sigma) or sigma.dim() != 3:
            raise ValueError('sigma must be a 3-D torch tensor on the GPU')
        k = _count('samples_per_cell', samples_per_cell, 1, MAX_SAMPLES_PER_CELL)
        rounds = _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS)
        threshold = _threshold(threshold)
        if not all((int(n) - 1) % k == 0 and int(n) > 1 for n in sigma.shape):
            raise ValueError(f'sigma {tuple(sigma.shape)}: every axis must hold cells * {k} + 1 points')
        cells = _cells([(int(n) - 1) // k for n in sigma.shape])
        lo, hi = mesh._bounds(bmin, bmax)
        words = ops.occupancy_build(sigma, cells, k, threshold)
        for _ in range(rounds):
            words = ops.occupancy_dilate(words, cells)
        return cls(lo, hi, cells, words)

    @classmethod
    def from_model(cls, render_kwargs, bmin, bmax, cells=128, threshold=DEFAULT_THRESHOLD, samples_per_cell=2, dilate=1,
                   networks=('coarse', 'fine'), chunk=1 << 18):
        """mesh.density_grid per network of `networks` at cells * samples_per_cell + 1 points per axis, from_density of
        each, and the OR of the resulting grids (the coarse pass is driven by the coarse network's sigma, the fine pass
        by the fine network's).  Refuses NDC-space models like density_grid."""
        cells = _cells(cells)
        k = _count('samples_per_cell', samples_per_cell, 1, MAX_SAMPLES_PER_CELL)
        threshold = _threshold(threshold)
        _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS)
        mesh._bounds(bmin, bmax)
        networks = tuple(networks)
        if not networks:
            raise ValueError("networks: at least one of 'coarse', 'fine'")
        for n in networks:
            mesh._network(render_kwargs, n)                               # ValueError for NDC models and unknown names
        words = None
        for n in networks:
            sigma = mesh.density_grid(render_kwargs, bmin, bmax, tuple(c * k + 1 for c in cells), network=n, chunk=chunk)
            g = cls.from_density(sigma, bmin, bmax, threshold, k, dilate)
            words = g.words if words is None else words | g.words
        return cls(bmin, bmax, cells, words)
