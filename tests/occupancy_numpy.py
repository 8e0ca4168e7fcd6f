"""numpy restatement of the occupancy grid (mvip_nerf_amd/occupancy.py, csrc/occupancy.hip), written from the
conventions alone -- the role tests/mc_numpy.py has for marching cubes.

Box [bmin, bmax], cells (cx, cy, cz); inv = cells / (bmax - bmin) formed in fp64 and rounded once to fp32.  Cell of a point
p, per axis in fp32: f = floor((p - bmin) * inv); inside the box iff 0 <= f < c on all three axes (NaN / inf: outside).
Linear cell l = (ix cy + iy) cz + iz, bit l & 31 of word l >> 5, unused tail bits zero.  keep(p) = outside, or bit set.
build: sigma [cx k + 1, cy k + 1, cz k + 1]; cell (i, j, l) owns points i k .. (i + 1) k inclusive per axis, occupied iff any
has !(sigma <= threshold).  dilate: occupied iff any cell at Chebyshev distance <= 1 is (clipped at the faces).
"""
import numpy as np


def inverse(bmin, bmax, cells):
    bmin, bmax = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
    return (np.asarray(cells, np.float64) / (bmax.astype(np.float64) - bmin.astype(np.float64))).astype(np.float32)


def n_words(cells):
    return (int(cells[0]) * int(cells[1]) * int(cells[2]) + 31) // 32


def pack(occ):
    """bool [cx, cy, cz] -> int32 words."""
    flat = np.asarray(occ, bool).reshape(-1)
    bits = np.zeros(n_words(occ.shape) * 32, np.uint8)
    bits[:flat.size] = flat
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').reshape(-1).view('<u4').astype(np.uint32).view(np.int32)


def unpack(words, cells):
    """int32 words -> bool [cx, cy, cz]; asserts the unused tail bits are zero."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32).astype('<u4')
    assert w.shape == (n_words(cells),)
    bits = np.unpackbits(w.view(np.uint8), bitorder='little')
    n = int(cells[0]) * int(cells[1]) * int(cells[2])
    assert not bits[n:].any(), 'tail bits must be zero'
    return bits[:n].astype(bool).reshape(cells)


def build(sigma, threshold, k=1):
    """bool [cx, cy, cz] from sigma [cx k + 1, cy k + 1, cz k + 1]."""
    sigma = np.asarray(sigma, np.float32)
    cells = tuple((n - 1) // k for n in sigma.shape)
    assert all(c * k + 1 == n and c >= 1 for c, n in zip(cells, sigma.shape))
    hit = ~(sigma <= np.float32(threshold))                         # NaN: the comparison is False, so the point counts
    occ = np.zeros(cells, bool)
    for a in range(k + 1):
        for b in range(k + 1):
            for c in range(k + 1):
                occ |= hit[a:a + cells[0] * k:k, b:b + cells[1] * k:k, c:c + cells[2] * k:k]
    return occ


def dilate(occ, rounds=1):
    occ = np.asarray(occ, bool)
    for _ in range(rounds):
        p = np.pad(occ, 1, constant_values=False)
        out = np.zeros_like(occ)
        cx, cy, cz = occ.shape
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    out |= p[dx:dx + cx, dy:dy + cy, dz:dz + cz]
        occ = out
    return occ


def cell_of(pts, bmin, bmax, cells):
    """(inside bool [P], linear cell int64 [P] (0 where outside)) of pts [P, 3], fp32 arithmetic as specified."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    bmin = np.asarray(bmin, np.float32)
    inv = inverse(bmin, bmax, cells)
    with np.errstate(invalid='ignore', over='ignore'):
        f = np.floor(((pts - bmin[None, :]).astype(np.float32) * inv[None, :]).astype(np.float32))
        c = np.asarray(cells, np.float32)[None, :]
        inside = np.all((f >= 0) & (f < c), axis=1)
    i = np.where(inside[:, None], f, 0).astype(np.int64)
    return inside, (i[:, 0] * int(cells[1]) + i[:, 1]) * int(cells[2]) + i[:, 2]


def keep(pts, bmin, bmax, cells, occ):
    """bool [P]: outside the box, or in an occupied cell."""
    inside, l = cell_of(pts, bmin, bmax, cells)
    return ~inside | np.asarray(occ, bool).reshape(-1)[l]
