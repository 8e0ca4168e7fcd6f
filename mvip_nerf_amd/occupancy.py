"""Occupancy grids for empty-space skipping in no-grad renders (beyond the reference: MVIP-NeRF evaluates every sample).

Rendering with a grid (`render_kwargs['occupancy'] = grid`, run.render_rays) means: the render the ordinary chain would
produce if the network's raw output were replaced by zeros (rgb_raw = 0, sigma = 0) at every sample whose point lies in a
cell the grid marks empty -- and the network is never evaluated at those samples.  A sample with sigma = 0 has alpha = 0 and
weight 0, so on a grid that is conservative the render equals the ordinary one; whether a grid is conservative is the
builder's business (from_density / from_model: threshold, samples_per_cell, dilate).

The grid is a bitgrid.BitGrid (the box, the cells and the word layout: bitgrid.py).  keep(p) = outside the box, or bit set:
points outside the box are always evaluated.  The kernels are csrc/occupancy.hip; there is no CPU path.
"""
import math

import torch

from . import mesh, ops
from .bitgrid import MAX_CELLS_PER_AXIS, BitGrid, _cells, _count

MAX_SAMPLES_PER_CELL = 8
# from_model's default: the largest threshold of tools/render_occupancy_ab.py's sweep that keeps the held-out PSNR of the
# 1,500-iteration scene-1 field within 0.05 dB of the ordinary render (profiles/occupancy_ab.json)
DEFAULT_THRESHOLD = 5.0


def _threshold(threshold):
    threshold = float(threshold)
    if not (threshold >= 0 and math.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and >= 0, got {threshold}')
    return threshold


class OccupancyGrid(BitGrid):
    """A BitGrid whose set bits are the occupied cells.  keep_components() (bitgrid.py) gives a grid without the dropped
    islands: rendering with it shows the scene WITHOUT them -- a different frame, the floaters gone from it, not merely
    skipped."""

    NOUN = 'an occupancy grid'

    def __init__(self, bmin, bmax, cells, words):
        super().__init__(bmin, bmax, cells, words)
        self.reset_stats()

    # -- bookkeeping of the renders that used this grid (run.render_rays adds to it) ----------------------------------
    def reset_stats(self):
        """stats: samples / kept samples per pass and the number of network launches, summed over the render_rays calls
        since the last reset."""
        self.stats = {'samples_coarse': 0, 'kept_coarse': 0, 'samples_fine': 0, 'kept_fine': 0, 'network_launches': 0}

    def occupied_fraction(self):
        return self.count() / self.n_cells

    def lookup(self, pts):
        """keep(p) of pts [..., 3] (device): bool [P], True = outside the box or in an occupied cell."""
        if not torch.is_tensor(pts) or pts.shape[-1] != 3:
            raise ValueError('pts must be a [..., 3] torch tensor on the GPU')
        if pts.device != self.words.device:
            raise ValueError(f'pts on {pts.device}, the grid on {self.words.device}')
        return ops.occupancy_lookup(pts, self.box(), self.cells, self.words).bool()

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
    def from_mesh(cls, mesh, bmin, bmax, cells=128, solid=True, dilate=1, margin=None):
        """The cells of a mesh.Mesh on the GPU as occupied cells (mesh.voxelize, csrc/mesh_voxel.hip), then `dilate` rounds
        of dilation: the cells the faces touch, and with solid=True the cells inside as well (column parity, the majority of
        three axes).  Like keep_components, and unlike from_model, this grid is NOT conservative for the field: a render with
        it shows the scene ONLY where the mesh is -- whatever the cleaned mesh no longer has (floaters, dropped interior,
        deselected components) is gone from the frame, not merely skipped, so the frame differs from the unskipped render.
        margin (scene units; None: no such step), applied after the voxelisation and before the dilation: > 0 also sets the
        cells whose centre lies within `margin` of the surface, < 0 clears them (mesh.margin_cells, csrc/mesh_sdf.hip)."""
        cells = _cells(cells)
        rounds = _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS)
        from .mesh import voxelize                                   # (the argument shadows the module here)
        from .mesh import apply_margin
        grid, _ = voxelize(mesh, bmin, bmax, cells, mode='both' if solid else 'surface')
        words = apply_margin(grid.words, mesh, grid.bmin, grid.bmax, cells, margin)
        for _ in range(rounds):
            words = ops.occupancy_dilate(words, cells)
        return cls(grid.bmin, grid.bmax, cells, words)

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
