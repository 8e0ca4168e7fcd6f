"""3D-consistent inpainting masks lifted from a few annotated views (beyond the reference: MVIP-NeRF takes one mask per
view as given and never says where they come from).

A *region* is a set of cells of a box: "the surfaces to be inpainted".  It is LIFTED from annotated 2D masks through the
trained field's own ray weights (Region.from_masks: the samples that carry the weight of the masked pixels' rays are
marked) and RENDERED into any view as the share of each ray's weight that falls inside it (run.render_rays' `region`
keyword -> 'region_map'; propagate_masks thresholds it).  A ray that is stopped by something in front of the region gets
no weight inside it: the masks are occlusion-aware.  Region.carve() gives the occupancy grid that renders the scene with
the region cut out -- the hole the inpainting has to fill.

The grid is a bitgrid.BitGrid, the one occupancy uses (the box, the cells and the word layout: bitgrid.py).  A sample's
point is row[0:3] + row[3:6] * z in the expression of the MLP ray kernels.  ONE difference, the reason for a type of its own:
inside(p) = in the box AND bit set (occupancy's keep(p) is "outside the box OR bit set").  The kernels are csrc/region.hip;
there is no CPU path.

Choosing the grid (from a CPU simulation of a ball in front of a wall, 64 + 64 samples): keep the cell edge above the
pixel footprint at the object's depth -- at 0.78 x the footprint the marked shell has holes and mask errors reach 4 cells,
at 1.5 x they stay under 0.6 cell -- and annotate a view from each side from which the object is seen: what the annotated
views cannot see (the limb of a ball) is not in the region.
"""
import numpy as np
import torch

from . import mesh, ops
from .bitgrid import MAX_CELLS_PER_AXIS, BitGrid, _cells, _count
from .occupancy import OccupancyGrid

KIND = 'region'


def default_box(lo, hi, cells, dilate):
    """The box from_points takes when none is given.  lo, hi [3]: the extent of the finite points.  Per axis e = hi - lo,
    h = e / (cells - 2 (dilate + 1)), bmin = lo - (dilate + 1) h, bmax = hi + (dilate + 1) h: the points fill the inner
    cells and no dilation round is clipped at a face.  ValueError when cells <= 2 (dilate + 1) or an extent is zero."""
    cells = _cells(cells)
    pad = _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS) + 1
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError('no finite point: the box cannot be derived from the points')
    if any(c <= 2 * pad for c in cells):
        raise ValueError(f'cells {cells} leave no inner cell with dilate = {pad - 1}: more than {2 * pad} cells per axis needed')
    if not np.all(hi > lo):
        raise ValueError(f'the points have zero extent on an axis (min {lo.tolist()}, max {hi.tolist()}): give bmin / bmax')
    h = (hi - lo) / (np.asarray(cells, np.float64) - 2 * pad)
    return (lo - pad * h).astype(np.float32), (hi + pad * h).astype(np.float32)


class Region(BitGrid):
    """A BitGrid whose set bits are the cells of the region; count() is their number.  keep_components() (bitgrid.py)
    gives a region whose isolated marked cells no longer count as inside."""

    KIND = KIND
    NOUN = 'a region'

    def fraction(self):
        """Share of the box's cells that are in the region."""
        return self.count() / self.n_cells

    def _same_device(self, t, what):
        if not torch.is_tensor(t):
            raise ValueError(f'{what} must be a torch tensor on the GPU')
        if t.device != self.words.device:
            raise ValueError(f'{what} on {t.device}, the region on {self.words.device}; use region.to(device)')

    def contains(self, pts):
        """inside(p) of pts [..., 3] (device): bool [P], True = in the box and in a cell of the region."""
        self._same_device(pts, 'pts')
        if pts.shape[-1] != 3:
            raise ValueError('pts must be a [..., 3] tensor')
        return ops.region_lookup(pts, self.box(), self.cells, self.words).bool()

    def accumulate(self, rows, z_vals, weights):
        """[B]: per ray, the sum of the weights of the samples inside the region (rows [B, 11], z_vals / weights [B, S]).
        Detached: carries no gradient."""
        self._same_device(rows, 'rows')
        if rows.dim() != 2 or rows.shape[1] != 11:
            raise ValueError(f'ray rows of 11 columns (with view directions, no depth column) expected, got {tuple(rows.shape)}')
        return ops.region_accumulate(rows, z_vals, weights, self.box(), self.cells, self.words)

    def dilate(self, rounds=1):
        """A new Region after `rounds` rounds of: in the region iff any cell at Chebyshev distance <= 1 is (clipped at the
        faces)."""
        words = self.words
        for _ in range(_count('dilate', rounds, 0, MAX_CELLS_PER_AXIS)):
            words = ops.occupancy_dilate(words, self.cells)
        return Region(self.bmin, self.bmax, self.cells, words.clone() if words is self.words else words)

    def carve(self):
        """occupancy.OccupancyGrid on the same box with the COMPLEMENT bits (tail bits zero).  Rendering with
        render_kwargs['occupancy'] = region.carve() skips exactly the samples inside the region: the scene with the region
        cut out, through the existing skipping route."""
        words = ~self.words
        tail = self.n_cells % 32
        if tail:
            words[-1] &= (1 << tail) - 1
        return OccupancyGrid(self.bmin, self.bmax, self.cells, words)

    @classmethod
    def from_points(cls, pts, bmin=None, bmax=None, cells=64, dilate=1):
        """The cells that hold a point of pts [P, 3] (device), then `dilate` rounds of dilation.  Points outside the box
        (NaN / inf included) mark nothing.  With no box given: default_box over the finite points."""
        if not torch.is_tensor(pts) or pts.shape[-1] != 3:
            raise ValueError('pts must be a [..., 3] torch tensor on the GPU')
        cells = _cells(cells)
        rounds = _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS)
        if (bmin is None) != (bmax is None):
            raise ValueError('give both bmin and bmax, or neither')
        pts = pts.reshape(-1, 3)
        if bmin is None:
            finite = pts[torch.isfinite(pts).all(-1)]
            if finite.shape[0] == 0:
                raise ValueError('no finite point: the box cannot be derived from the points')
            bmin, bmax = default_box(finite.min(0).values.cpu().numpy(), finite.max(0).values.cpu().numpy(), cells, rounds)
        r = cls(bmin, bmax, cells, torch.zeros(ops.occupancy_words(cells), device=pts.device, dtype=torch.int32))
        ops.region_mark(pts, r.box(), r.cells, r.words)
        return r.dilate(rounds)

    @classmethod
    def from_mesh(cls, mesh, bmin=None, bmax=None, cells=64, solid=True, dilate=1, margin=None):
        """The cells of a mesh (mesh.voxelize, csrc/mesh_voxel.hip), then `dilate` rounds of dilation: with solid=True the
        cells the faces touch and the cells inside (column parity, the majority of three axes: a hole in the mesh leaks
        nothing beyond the missing faces' own cells), with solid=False the surface cells only.  mesh: a mesh.Mesh on the
        GPU, for instance one component picked by mesh.keep_components(containing=...).  With no box given: default_box over
        the finite vertices, as from_points.  The region renders into every view as an occlusion-aware mask (propagate_masks)
        and carve() cuts it out of the scene.
        margin (scene units; None: no such step), applied after the voxelisation and before the dilation: > 0 also sets every
        cell whose centre lies within `margin` of the surface -- the halo and the contact shadow round an object, by a
        distance and not by whole cells; < 0 clears those cells, which peels a solid region by |margin| (mesh.margin_cells,
        csrc/mesh_sdf.hip).  A box derived here is not grown by the margin: give one that holds it."""
        cells = _cells(cells)
        rounds = _count('dilate', dilate, 0, MAX_CELLS_PER_AXIS)
        if (bmin is None) != (bmax is None):
            raise ValueError('give both bmin and bmax, or neither')
        if bmin is None:
            v = mesh.verts.detach().reshape(-1, 3)
            finite = v[torch.isfinite(v).all(-1)]
            if finite.shape[0] == 0:
                raise ValueError('no finite vertex: the box cannot be derived from the mesh')
            bmin, bmax = default_box(finite.min(0).values.cpu().numpy(), finite.max(0).values.cpu().numpy(), cells, rounds)
        from .mesh import voxelize                                   # (the argument shadows the module here)
        from .mesh import apply_margin
        grid, _ = voxelize(mesh, bmin, bmax, cells, mode='both' if solid else 'surface')
        words = apply_margin(grid.words, mesh, grid.bmin, grid.bmax, cells, margin)
        return cls(grid.bmin, grid.bmax, cells, words).dilate(rounds)

    @classmethod
    def from_masks(cls, render_kwargs, hwf, poses, masks, near, far, bmin=None, bmax=None, cells=64, min_weight=None,
                   dilate=1, chunk=1 << 15):
        """Lift masks [V, H, W] (bool; poses [V, 3, 4] camera-to-world) into a region.  Per annotated view, under
        torch.no_grad(), only the masked pixels are rendered with the test-time kwargs; of the final pass (fine if
        N_importance > 0) the samples with weights >= min_weight are selected (a NaN weight fails), their points are formed
        and marked; the union over the views goes through from_points (box rule, dilation).

        min_weight defaults to 1 / S, S = samples of the final pass: a sample is marked iff it carries more than the
        uniform share of an opaque ray.  That is a definition, not a tuned value; raise or lower it for fields that are
        crisper or foggier.  What is marked is the VISIBLE SHELL: the surfaces seen through masked pixels.  Background seen
        through the rim of a generous mask is marked too, and is then masked in every view where it is visible -- that is
        the meaning of "3D-consistent".

        ValueError: NDC-space models, models without view directions, raw_noise_std > 0, masks that are not [V, H, W] for
        the V poses, no marked sample at all."""
        from . import run
        mesh._network(render_kwargs, 'fine')                                     # ValueError for NDC models
        if not render_kwargs.get('use_viewdirs', True):
            raise ValueError('from_masks: a model with view directions is expected (ray rows of 11 columns)')
        if render_kwargs.get('raw_noise_std', 0.) > 0.:
            raise ValueError('from_masks: raw_noise_std > 0 perturbs the weights that are lifted; use the test-time kwargs')
        H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
        poses = torch.as_tensor(poses)
        masks = torch.as_tensor(masks)
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or tuple(masks.shape) != (poses.shape[0], H, W):
            raise ValueError(f'poses [V, 3, 4] and masks [V, {H}, {W}] expected, got {tuple(poses.shape)} and '
                             f'{tuple(masks.shape)}')
        if min_weight is not None and not float(min_weight) > 0:
            raise ValueError(f'min_weight must be > 0, got {min_weight}')
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError('chunk must be >= 1')
        kw = {k: v for k, v in render_kwargs.items() if k not in ('ndc', 'use_viewdirs', 'near', 'far', 'region')}
        marked = []
        with torch.no_grad():
            for c2w, mask in zip(poses, masks):
                idx = torch.nonzero(mask.reshape(-1) != 0).reshape(-1).to(c2w.device)
                for s in range(0, idx.shape[0], chunk):
                    rows = ops.ray_rows_from_pose(c2w, H, W, focal, near, far, sel=idx[s:s + chunk])
                    ret = run.batchify_rays(rows, chunk, **kw)
                    w, z = ret['weights'], ret['z_vals']
                    thr = 1.0 / z.shape[1] if min_weight is None else float(min_weight)
                    pts = rows[:, None, 0:3] + rows[:, None, 3:6] * z[:, :, None]
                    marked.append(pts[w >= float(np.float32(thr))])
        n = sum(p.shape[0] for p in marked)
        if n == 0:
            raise ValueError('from_masks: no sample of a masked ray reaches min_weight (empty masks, or an empty field '
                             'behind them): nothing to lift')
        return cls.from_points(torch.cat(marked, 0), bmin, bmax, cells, dilate)


def propagate_masks(render_kwargs, hwf, poses, region, near, far, threshold=0.5, chunk=1 << 15):
    """(soft float32 [N, H, W], hard bool [N, H, W]) for poses [N, 3, 4]: soft = the 'region_map' of a no-grad render of each
    pose (the share of each ray's weight inside the region), hard = soft >= threshold."""
    from . import run
    if not isinstance(region, Region):
        raise ValueError(f'region must be a region.Region, got {type(region).__name__}')
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    poses = torch.as_tensor(poses)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f'poses [N, 3, 4] expected, got {tuple(poses.shape)}')
    kw = dict(render_kwargs, near=near, far=far, region=region)
    soft = []
    with torch.no_grad():
        for c2w in poses:
            soft.append(run.render(H, W, focal, chunk=int(chunk), c2w=c2w, **kw)[4]['region_map'])
    soft = torch.stack(soft, 0) if soft else torch.empty((0, H, W), device=region.device)
    return soft, soft >= float(threshold)
