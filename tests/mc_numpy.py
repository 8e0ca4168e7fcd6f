"""Vectorised numpy restatement of the marching-cubes passes of csrc/mcubes.hip (TEST HELPER, not collected): the same
conventions and the same triangle table (mvip_nerf_amd.mesh.TRI_TABLE), in fp32 arithmetic in the kernels' operation
order, plus mesh checks (edge incidence, Euler characteristic, signed volume) and a reader for save_ply's files."""
import numpy as np

from mvip_nerf_amd.mesh import TRI_TABLE

TABLE = np.array(TRI_TABLE, dtype=np.int64)                       # [256, 16]
COUNTS = (TABLE[:, 0::3][:, :5] >= 0).sum(1)                     # triangles per cube index
F32 = np.float32


def _grad(v, axis, h):
    """d v / d axis: central differences inside, one-sided on the grid's faces, (v[hi] - v[lo]) / ((hi - lo) * h)."""
    n = v.shape[axis]
    idx = np.arange(n)
    lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
    num = np.take(v, hi, axis) - np.take(v, lo, axis)
    den = ((hi - lo).astype(F32) * F32(h)).astype(F32)
    shape = [1, 1, 1]
    shape[axis] = n
    return (num / den.reshape(shape)).astype(F32)


def marching_cubes(grid, iso, bmin, bmax):
    """-> verts [V, 3] f32, faces [F, 3] int64, normals [V, 3] f32 (same order as the kernels)."""
    v = np.ascontiguousarray(grid, dtype=F32)
    nx, ny, nz = v.shape
    lo, hi = np.asarray(bmin, F32), np.asarray(bmax, F32)
    iso = F32(iso)
    h = ((hi - lo) / np.array([nx - 1, ny - 1, nz - 1], F32)).astype(F32)
    ins = v >= iso
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    mask = (cross[..., 0] * 1 + cross[..., 1] * 2 + cross[..., 2] * 4).reshape(-1)
    counts = cross.reshape(-1, 3).sum(1)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    # vertices, (point, axis) order
    pt, ax = np.nonzero(cross.reshape(-1, 3))
    i, j, k = np.unravel_index(pt, v.shape)
    d = np.eye(3, dtype=np.int64)[ax]
    i1, j1, k1 = i + d[:, 0], j + d[:, 1], k + d[:, 2]
    v0, v1 = v[i, j, k], v[i1, j1, k1]
    t = ((iso - v0) / (v1 - v0)).astype(F32)
    p0 = np.stack([lo[0] + i.astype(F32) * h[0], lo[1] + j.astype(F32) * h[1], lo[2] + k.astype(F32) * h[2]], -1)
    p1 = np.stack([lo[0] + i1.astype(F32) * h[0], lo[1] + j1.astype(F32) * h[1], lo[2] + k1.astype(F32) * h[2]], -1)
    verts = (p0 + t[:, None] * (p1 - p0)).astype(F32)
    G = [_grad(v, a, h[a]) for a in range(3)]
    g0 = np.stack([G[a][i, j, k] for a in range(3)], -1)
    g1 = np.stack([G[a][i1, j1, k1] for a in range(3)], -1)
    g = (g0 + t[:, None] * (g1 - g0)).astype(F32)
    ln = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(ln[:, None] > 0, -g / ln[:, None], F32(0)).astype(F32)
    # triangles, (cell, slot) order; cells indexed by their origin point
    c = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for corner in range(8):
        dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
        c |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << corner
    ci, cj, ck = np.nonzero(COUNTS[c] > 0)
    cube = c[ci, cj, ck]
    cell = np.ravel_multi_index((ci, cj, ck), v.shape)
    nt = COUNTS[cube]
    rep = np.repeat(np.arange(cube.shape[0]), nt)
    slot = np.arange(rep.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)
    e = TABLE[cube[rep][:, None], 3 * slot[:, None] + np.arange(3)[None]]      # [F, 3] edge numbers
    a, r1, r2 = e >> 2, e & 1, (e >> 1) & 1
    dx = np.where(a == 0, 0, r1)
    dy = np.where(a == 1, 0, np.where(a == 0, r1, r2))
    dz = np.where(a == 2, 0, r2)
    m = cell[rep][:, None] + dx * ny * nz + dy * nz + dz
    below = mask[m] & ((1 << a) - 1)
    rank = (below & 1) + ((below >> 1) & 1)
    faces = first[m] + rank
    return verts, faces.astype(np.int64), normals


def cube_indices(grid, iso):
    """cube index of every cell (for coverage checks)."""
    ins = np.asarray(grid) >= iso
    nx, ny, nz = ins.shape
    c = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for corner in range(8):
        dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
        c |= ins[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << corner
    return c


def edge_incidence(faces):
    """undirected edges [E, 2] and the number of faces each is in."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e.sort(1)
    return np.unique(e, axis=0, return_counts=True)


def directed_edges_paired(faces):
    """True when every directed edge (a, b) of the faces appears once and its reverse (b, a) once: consistently oriented."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = e[:, 0] * (int(f.max()) + 1) + e[:, 1]
    rkey = e[:, 1] * (int(f.max()) + 1) + e[:, 0]
    return np.unique(key).shape[0] == key.shape[0] and np.array_equal(np.sort(key), np.sort(rkey))


def euler(verts, faces):
    edges, _ = edge_incidence(faces)
    return len(verts) - len(edges) + len(faces)


def signed_volume(verts, faces):
    p = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(np.einsum('fi,fi->f', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def is_closed(faces):
    _, n = edge_incidence(faces)
    return bool(np.all(n == 2)) and directed_edges_paired(faces)


def read_ply(path):
    """(header lines, vertex structured array, faces [F, 3] int32) of a binary little-endian PLY as save_ply writes it."""
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').strip().split('\n')
    assert head[0] == 'ply' and head[1] == 'format binary_little_endian 1.0'
    nv = nf = None
    vprops = []
    cur = None
    for line in head:
        w = line.split()
        if w[0] == 'element':
            cur = w[1]
            if cur == 'vertex':
                nv = int(w[2])
            elif cur == 'face':
                nf = int(w[2])
        elif w[0] == 'property' and cur == 'vertex':
            vprops.append((w[2], {'float': '<f4', 'uchar': 'u1'}[w[1]]))
        elif w[0] == 'property' and cur == 'face':
            assert w[1:4] == ['list', 'uchar', 'int']
    vert = np.frombuffer(data, dtype=vprops, count=nv, offset=end)
    off = end + vert.nbytes
    face = np.frombuffer(data, dtype=[('n', 'u1'), ('v', '<i4', (3,))], count=nf, offset=off)
    assert off + face.nbytes == len(data)
    assert np.all(face['n'] == 3)
    return head, vert, face['v'].copy()
