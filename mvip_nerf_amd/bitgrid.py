"""The bit grid that occupancy.OccupancyGrid and region.Region share: one bit per cell of an axis-aligned box.

THE statement of the convention on the Python side (device side: csrc/bitgrid_device.h; restated for the tests in
tests/occupancy_numpy.py and tests/region_numpy.py): box [bmin, bmax], cells = (cx, cy, cz), each 1..512; inv = cells /
(bmax - bmin), formed once in fp64 and rounded to fp32.  Cell of a point p, per axis in fp32: f = floorf((p - bmin) * inv);
p is in the box iff 0 <= f < c on all three axes (a NaN or infinite coordinate fails the comparison: outside).  Linear cell
l = (ix * cy + iy) * cz + iz (z fastest, like mesh.py), bit l & 31 of int32 word l >> 5, unused tail bits zero.  What a
clear bit or a point outside the box MEANS is the subclass's: occupancy's keep(p), region's inside(p).  There is no CPU
path: the words live on the device.
"""
import numpy as np
import torch

from . import mesh, ops

MAX_CELLS_PER_AXIS = 512
FORMAT_VERSION = 1


def _cells(cells):
    c = (int(cells),) * 3 if np.isscalar(cells) else tuple(int(n) for n in cells)
    if len(c) != 3 or not all(1 <= n <= MAX_CELLS_PER_AXIS for n in c):
        raise ValueError(f'cells {c}: three axes of 1..{MAX_CELLS_PER_AXIS} cells each')
    return c


def _count(name, v, lo, hi):
    if int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f'{name} must be an integer in {lo}..{hi}, got {v!r}')
    return int(v)


def cell_inverse(bmin, bmax, cells):
    """inv [3] fp32 = cells / (bmax - bmin), the quotient formed in fp64 and rounded once."""
    return (np.asarray(cells, np.float64) / (bmax.astype(np.float64) - bmin.astype(np.float64))).astype(np.float32)


class BitGrid:
    """One bit per cell of an axis-aligned box.  `words`: int32 [(cx cy cz + 31) // 32] on the device the grid is used on
    (a numpy array or CPU tensor is accepted where no kernel is called: save / load / count)."""

    KIND = None                    # the 'kind' key of the .npz; None: the file has none (and load does not look for one)
    NOUN = 'a bit grid'            # what the messages of load call the file

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
        return type(self)(self.bmin, self.bmax, self.cells, self.words.to(device))

    def count(self):
        """Number of set bits."""
        w = self.words.detach().cpu().numpy().view(np.uint32)
        return int(np.unpackbits(w.view(np.uint8)).sum())

    def components(self, connectivity=6):
        """Connected components of the set cells (ops.grid_components, csrc/components.hip): (labels [cx, cy, cz] int32,
        sizes [n] int32, first [n] int32), all on the grid's device.  labels is 0 for a clear bit, else the 1-based number
        of the cell's component, numbered by ascending lowest linear cell (`first`).  connectivity: 6 (cells that share a
        face) or 26 (a face, an edge or a corner)."""
        return ops.grid_components(self.words, self.cells, connectivity)

    def _labels_at(self, labels, pts):
        """Labels of the cells that pts [P, 3] fall in (cell_of's convention, in fp32 on the device); points outside the
        box are left out."""
        pts = torch.as_tensor(pts, dtype=torch.float32).reshape(-1, 3).to(self.device)
        bmin = torch.from_numpy(self.bmin).to(self.device)
        inv = torch.from_numpy(self.inv).to(self.device)
        c = torch.tensor(self.cells, dtype=torch.float32, device=self.device)
        f = torch.floor((pts - bmin) * inv)
        inside = ((f >= 0) & (f < c)).all(-1)
        i = f[inside].to(torch.int64)
        return labels.reshape(-1)[(i[:, 0] * self.cells[1] + i[:, 1]) * self.cells[2] + i[:, 2]]

    def keep_components(self, largest=None, min_cells=None, containing=None, connectivity=6):
        """A new grid of the same type and box whose set bits are those of the kept components only.

        largest = k: the k components with the most cells (ties: the lower `first`).  min_cells = m: components of at
        least m cells.  Each of the two restricts the kept set: a component must meet both where both are given.
        containing = pts [P, 3]: the components of the cells those points fall in (points outside the box or in a clear
        cell name none), kept IN ADDITION to the restricted set.  ValueError for no criterion, k < 1 or m < 1.  The kept
        set is chosen on the host from sizes / first (one small copy); the bits are written by ops.grid_select.

        What dropping a component means is the subclass's.  An OccupancyGrid without its small islands renders the scene
        WITHOUT them: the floaters are gone from the frame, not merely skipped, so the frame differs from the unskipped
        render (unlike the grid from_model builds, which only skips what contributes nothing).  A Region without its
        isolated cells no longer counts them as inside: stray marks far from the object stop masking pixels."""
        if connectivity not in ops.CONNECTIVITIES:
            raise ValueError(f'keep_components: connectivity must be 6 or 26, got {connectivity!r}')
        largest, min_cells = ops.component_criteria('keep_components', largest, min_cells, containing is not None)
        labels, sizes, _ = self.components(connectivity)
        also = None if containing is None else self._labels_at(labels, containing).cpu().numpy()
        keep = ops.component_keep_table(sizes.cpu().numpy(), largest, min_cells, also)
        words = ops.grid_select(labels, torch.from_numpy(keep).to(self.device))
        return type(self)(self.bmin, self.bmax, self.cells, words)

    def save(self, path):
        """An .npz of the words and the five small arrays (bmin, bmax, cells, inv, version), plus `kind` where the class
        has one."""
        kind = {} if self.KIND is None else {'kind': np.asarray(self.KIND)}
        np.savez(path, words=self.words.detach().cpu().numpy(), bmin=self.bmin, bmax=self.bmax,
                 cells=np.asarray(self.cells, np.int32), inv=self.inv, version=np.asarray([FORMAT_VERSION], np.int32), **kind)

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as d:
            missing = [k for k in ('words', 'bmin', 'bmax', 'cells', 'inv', 'version') if k not in d.files]
            if missing:
                raise ValueError(f'{path}: not {cls.NOUN} file (missing {missing})')
            if cls.KIND is not None and ('kind' not in d.files or str(d['kind']) != cls.KIND):
                raise ValueError(f"{path}: not {cls.NOUN} file (no kind = '{cls.KIND}'; an occupancy grid means the opposite "
                                 f'outside its box and is not read as {cls.NOUN})')
            if int(d['version'][0]) != FORMAT_VERSION:
                raise ValueError(f'{path}: format version {int(d["version"][0])}, expected {FORMAT_VERSION}')
            words, bmin, bmax, cells, inv = d['words'], d['bmin'], d['bmax'], d['cells'], d['inv']
        g = cls(bmin, bmax, tuple(int(c) for c in cells), torch.from_numpy(words.astype(np.int32, copy=False)))
        if not np.array_equal(g.inv, inv.astype(np.float32)):
            raise ValueError(f'{path}: stored cell scale {inv.tolist()} differs from the one its box gives {g.inv.tolist()}')
        return g if device is None else g.to(device)
