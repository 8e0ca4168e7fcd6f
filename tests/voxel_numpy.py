"""The restatement of csrc/mesh_voxel.hip for the tests: mesh voxelisation by brute force in numpy, fp64 and integers, every
expression associated as the kernel's header writes it, so that the GPU result can be compared BIT FOR BIT.

Lattice coordinates: g = (double(p) - double(bmin)) * double(inv) per axis; cell i spans [i, i + 1), centre i + 0.5; linear cell
l = (ix cy + iy) cz + iz, bit l & 31 of word l >> 5, tail bits zero.

SOLID (parity fill).  Column axis a, raster axes (b, c) = (y, z), (z, x), (x, y).  A face is dropped whole, and counted once,
unless all nine g are finite and |256 g| <= 2^22 on every raster axis of every walked axis.  X = rint(256 g_b), Y = rint(256 g_c);
A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); A2 = 0: skipped for the axis; A2 < 0: vertices 1 and 2 swapped.  The sample of
column (x, y) is (256 x + 128, 256 y + 128); E_k = ex (sy - Yi) - ey (sx - Xi) for the edge i -> j opposite k; covered iff every
E_k > 0, or E_k = 0 and (ey < 0, or ey = 0 and ex > 0).  depth = ((E0 g0_a + E1 g1_a) + E2 g2_a) / A2; k = floor(depth - 0.5) + 1;
k >= cells_a: no mark; k < 0: k = 0; one crossing bit XORed at (x, y, k).  Inside iff the XOR of the crossing bits 0..i is 1;
odd_columns[a] = columns of odd total parity.  'majority': at least two of three.  Here EVERY column of the grid is tested against
EVERY face (no bounding box).

SURFACE (conservative).  m = 2^-12; a face with a non-finite g is dropped and counted.  Candidates per axis floor(min g - m) ..
floor(max g + m) clipped to the grid; e0 = g1 - g0, e1 = g2 - g1, e2 = g0 - g2, n = e0 x e1; v_k = g_k - centre, h = 0.5 + m; set
iff neither the normal (|(n_x v0x + n_y v0y) + n_z v0z| > h ((|n_x| + |n_y|) + |n_z|)) nor one of the nine unit_i x e_j (p_k over
the three vertices, separated iff min p > r or max p < -r; unit_x: p = e_y v_z - e_z v_y, r = h (|e_y| + |e_z|); unit_y:
p = e_z v_x - e_x v_z, r = h (|e_z| + |e_x|); unit_z: p = e_x v_y - e_y v_x, r = h (|e_x| + |e_y|)) separates.
"""
import numpy as np

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
BAND = 4194304.0
MARGIN = 1.0 / 4096.0
AXES = ('x', 'y', 'z', 'majority')


def grid_box(bmin, bmax, cells):
    """(bmin[3], inv[3]) as six fp32 numbers, as bitgrid.BitGrid.box() forms them: inv = cells / (bmax - bmin) in fp64, rounded once"""
    lo, hi = np.asarray(bmin, F32), np.asarray(bmax, F32)
    inv = (np.asarray(cells, F64) / (hi.astype(F64) - lo.astype(F64))).astype(F32)
    return [float(x) for x in lo] + [float(x) for x in inv]


def lattice(verts, box):
    b = np.asarray(box, F32).astype(F64)
    with np.errstate(all='ignore'):
        return (np.asarray(verts, F32).astype(F64).reshape(-1, 3) - b[:3]) * b[3:]


def pack(bits):
    """bool [cx, cy, cz] -> int32 words"""
    flat = np.asarray(bits, bool).reshape(-1)
    pad = (-len(flat)) % 32
    flat = np.concatenate([flat, np.zeros(pad, bool)])
    return np.packbits(flat, bitorder='little').view(np.uint32).astype(np.uint32).view(I32)


def unpack(words, cells):
    """int32 words -> bool [cx, cy, cz]; the tail bits must be zero"""
    n = int(cells[0]) * int(cells[1]) * int(cells[2])
    bits = np.unpackbits(np.ascontiguousarray(np.asarray(words, I32)).view(np.uint8), bitorder='little').astype(bool)
    assert len(bits) == (n + 31) // 32 * 32 and not bits[n:].any()
    return bits[:n].reshape(tuple(int(c) for c in cells))


def centres(box, cells):
    """world positions [cx, cy, cz, 3] fp64 of the cell centres (for the tests' first-principles checks, not for bits)"""
    b = np.asarray(box, F32).astype(F64)
    ax = [b[a] + (np.arange(cells[a], dtype=F64) + 0.5) / b[3 + a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1)


def _finite(G):
    return bool(np.all(np.abs(G) <= 1.7976931348623157e308))


def solid_axis(g, faces, cells, a, kept):
    """(inside bool [cx, cy, cz], odd_columns) of column axis a over the faces kept[f]"""
    b, c = (a + 1) % 3, (a + 2) % 3
    ca, cb, cc = (int(cells[k]) for k in (a, b, c))
    cross = np.zeros((cb, cc, ca), bool)
    sx = (256 * np.arange(cb, dtype=I64) + 128)[:, None]
    sy = (256 * np.arange(cc, dtype=I64) + 128)[None, :]
    for fi in np.nonzero(kept)[0]:
        G = g[faces[fi]]
        X = np.rint(256.0 * G[:, b]).astype(I64)
        Y = np.rint(256.0 * G[:, c]).astype(I64)
        d = G[:, a].copy()
        A2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if A2 == 0:
            continue
        if A2 < 0:
            X[[1, 2]], Y[[1, 2]], d[[1, 2]] = X[[2, 1]], Y[[2, 1]], d[[2, 1]]
            A2 = -A2
        E, covered = [], np.ones((cb, cc), bool)
        for i, j in ((1, 2), (2, 0), (0, 1)):
            ex, ey = X[j] - X[i], Y[j] - Y[i]
            Ek = ex * (sy - Y[i]) - ey * (sx - X[i])
            owns = bool(ey < 0 or (ey == 0 and ex > 0))
            covered &= (Ek > 0) | ((Ek == 0) & owns)
            E.append(Ek.astype(F64))
        depth = ((E[0] * d[0] + E[1] * d[1]) + E[2] * d[2]) / F64(A2)
        k = np.floor(depth - 0.5) + 1.0
        mark = covered & (k < ca)
        xs, ys = np.nonzero(mark)
        ks = np.where(k[xs, ys] < 0.0, 0.0, k[xs, ys]).astype(I64)
        cross[xs, ys, ks] ^= True                                # one sample per column and face: no index repeats
    inside = np.logical_xor.accumulate(cross, axis=2)
    odd = int(inside[:, :, -1].sum())
    return inside.transpose({0: (2, 0, 1), 1: (1, 2, 0), 2: (0, 1, 2)}[a]), odd


def kept_faces(g, faces, axes):
    """bool [F]: not DROPPED WHOLE"""
    walked = (0, 1, 2) if axes == 'majority' else (AXES.index(axes),)
    guard = sorted({k for a in walked for k in ((a + 1) % 3, (a + 2) % 3)})
    out = np.zeros(len(faces), bool)
    for fi, f in enumerate(faces):
        G = g[f]
        out[fi] = _finite(G) and bool(np.all(np.abs(256.0 * G[:, guard]) <= BAND))
    return out


def solid(verts, faces, box, cells, axes='majority'):
    """(words int32, odd_columns [3], dropped, per_axis {a: bool [cx, cy, cz]})"""
    assert axes in AXES
    faces = np.asarray(faces, I64).reshape(-1, 3)
    g = lattice(verts, box)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(g))
    kept = kept_faces(g, faces, axes)
    walked = (0, 1, 2) if axes == 'majority' else (AXES.index(axes),)
    per, odd = {}, [0, 0, 0]
    for a in walked:
        per[a], odd[a] = solid_axis(g, faces, cells, a, kept)
    if axes == 'majority':
        bits = (per[0].astype(I32) + per[1] + per[2]) >= 2
    else:
        bits = per[walked[0]]
    return pack(bits), odd, int(len(faces) - kept.sum()), per


def _separated(p0, p1, p2, r):
    return (np.minimum(p0, np.minimum(p1, p2)) > r) | (np.maximum(p0, np.maximum(p1, p2)) < -r)


def surface(verts, faces, box, cells):
    """(words int32, dropped)"""
    faces = np.asarray(faces, I64).reshape(-1, 3)
    g = lattice(verts, box)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(g))
    cells = tuple(int(c) for c in cells)
    out = np.zeros(cells, bool)
    dropped = 0
    h = 0.5 + MARGIN
    for f in faces:
        G = g[f]
        if not _finite(G):
            dropped += 1
            continue
        lo = np.maximum(np.floor(G.min(0) - MARGIN), 0.0)
        hi = np.minimum(np.floor(G.max(0) + MARGIN), np.asarray(cells, F64) - 1.0)
        if not np.all(lo <= hi):
            continue
        lo, hi = lo.astype(I64), hi.astype(I64)
        cx, cy, cz = np.meshgrid(*[np.arange(lo[a], hi[a] + 1, dtype=F64) + 0.5 for a in range(3)], indexing='ij')
        e = [G[1] - G[0], G[2] - G[1], G[0] - G[2]]
        n = (e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0])
        v = [(G[k][0] - cx, G[k][1] - cy, G[k][2] - cz) for k in range(3)]
        sep = np.abs((n[0] * v[0][0] + n[1] * v[0][1]) + n[2] * v[0][2]) > h * ((abs(n[0]) + abs(n[1])) + abs(n[2]))
        for ex, ey, ez in e:
            sep |= _separated(*[ey * v[k][2] - ez * v[k][1] for k in range(3)], h * (abs(ey) + abs(ez)))
            sep |= _separated(*[ez * v[k][0] - ex * v[k][2] for k in range(3)], h * (abs(ez) + abs(ex)))
            sep |= _separated(*[ex * v[k][1] - ey * v[k][0] for k in range(3)], h * (abs(ex) + abs(ey)))
        out[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= ~sep
    return pack(out), dropped


def cell_of(points, box, cells):
    """bitgrid's cell_of in fp32: (ix, iy, iz) int64 [P, 3] and in_box [P]"""
    b = np.asarray(box, F32)
    with np.errstate(all='ignore'):
        f = np.floor((np.asarray(points, F32) - b[:3]) * b[3:])
    inside = np.all((f >= 0) & (f < np.asarray(cells, F32)), -1)
    return np.where(inside[:, None], f, 0).astype(I64), inside


# ---- meshes for the tests -------------------------------------------------------------------------------------------------
def box_mesh(lo, hi, flip=False):
    """the axis-aligned box [lo, hi]: 8 vertices, 12 outward triangles (inward with flip)"""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    s = np.asarray([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F64)
    v = (lo + s * (hi - lo)).astype(F32)
    f = np.asarray([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                    (1, 5, 7), (1, 7, 3)], I32)
    return v, (f[:, ::-1].copy() if flip else f)


def tie_mesh(flip=False):
    """(verts, faces, box, cells): a box whose corners sit exactly at cell centres of the lattice bmin = 0, inv = 1, cells
    (8, 7, 6): its edges run through samples, its faces lie at centre depth"""
    v, f = box_mesh((1.5, 1.5, 1.5), (5.5, 4.5, 3.5), flip)
    return v, f, [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], (8, 7, 6)


def polyhedron_volume(verts, faces):
    """signed tetrahedra against the origin, fp64"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, I64)
    return float(np.sum(np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))) / 6.0)


def radii(verts, faces):
    """(inscribed, circumscribed) radius about the origin of a convex polyhedron that contains it: the smallest plane distance of
    a face and the largest vertex norm"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, I64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(np.min(np.einsum('ij,ij->i', n, v[f[:, 0]]))), float(np.max(np.linalg.norm(v, axis=1)))
