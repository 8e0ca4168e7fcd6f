"""Mesh export without a GPU: the triangle table of mvip_nerf_amd/mesh.py checked on the numpy restatement of the
marching-cubes passes (tests/mc_numpy.py), save_ply / frustum_bounds, the argument checks of the three mvip_mcubes_*
entry points (MVIP_EINVAL / MVIP_OK / MVIP_EINVAL as in tests/test_abi_errors.py) and the Python-level argument errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402

from mvip_nerf_amd import _lib, mesh                     # noqa: E402


def lattice(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n, dtype=np.float32)
    return np.meshgrid(x, x, x, indexing='ij')


def sphere_grid(n=65, r=0.6):
    X, Y, Z = lattice(n)
    return (2.0 - np.sqrt(X * X + Y * Y + Z * Z) / r).astype(np.float32)          # inside iff >= 1


def test_table_shape_and_orientation_rule():
    t = np.array(mesh.TRI_TABLE)
    assert t.shape == (256, 16)
    assert np.all(t[0] == -1) and np.all(t[255] == -1)
    for row in t:
        k = int(np.argmax(row < 0))
        assert k % 3 == 0 and k <= 15 and np.all(row[k:] == -1) and np.all((row[:k] >= 0) & (row[:k] < 12))
    assert M.COUNTS.max() == 5


def test_sphere_closed_euler_volume():
    r = 0.6
    v, f, nrm = M.marching_cubes(sphere_grid(65, r), 1.0, (-1, -1, -1), (1, 1, 1))
    edges, inc = M.edge_incidence(f)
    assert np.all(inc == 2)
    assert M.directed_edges_paired(f)
    assert len(v) - len(edges) + len(f) == 2
    vol = M.signed_volume(v, f)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * r ** 3) <= 0.01 * 4 / 3 * np.pi * r ** 3
    assert np.max(np.abs(np.linalg.norm(v, axis=1) - r)) <= 0.01
    assert np.all(np.einsum('ij,ij->i', nrm, v) > 0)                    # normals point outward


def test_torus_closed_genus_one():
    X, Y, Z = lattice(49)
    R, r = 0.55, 0.22
    g = (2.0 - np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) / r).astype(np.float32)
    v, f, _ = M.marching_cubes(g, 1.0, (-1, -1, -1), (1, 1, 1))
    assert M.is_closed(f)
    assert M.euler(v, f) == 0
    vol = M.signed_volume(v, f)
    assert abs(vol - 2 * np.pi ** 2 * R * r ** 2) <= 0.02 * 2 * np.pi ** 2 * R * r ** 2


def _ambiguous_faces(cube):
    """(axis, side, diagonal) of each face of cube index `cube` whose two inside corners sit on a diagonal."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for side in range(2):
            corners = [((side << a) | (u << b) | (w << c)) for u in (0, 1) for w in (0, 1)]   # (0,0) (0,1) (1,0) (1,1)
            ins = [(cube >> q) & 1 for q in corners]
            if ins == [1, 0, 0, 1]:
                out.append((a, side, 0))
            elif ins == [0, 1, 1, 0]:
                out.append((a, side, 1))
    return out


def test_random_fields_closed_and_cover_every_ambiguous_face():
    seen_faces, seen_cubes = set(), set()
    for seed in range(20):
        rs = np.random.RandomState(seed)
        g = rs.choice(np.array([-1.0, 1.0], np.float32), size=(12, 12, 12))
        g[[0, -1], :, :] = -1.0
        g[:, [0, -1], :] = -1.0
        g[:, :, [0, -1]] = -1.0
        v, f, _ = M.marching_cubes(g, 0.5, (0, 0, 0), (1, 1, 1))
        assert M.is_closed(f), seed
        assert M.signed_volume(v, f) > 0
        cubes = set(np.unique(M.cube_indices(g, 0.5)).tolist())
        seen_cubes |= cubes
        for cube in cubes:
            seen_faces |= set(_ambiguous_faces(cube))
    assert seen_faces == {(a, s, d) for a in range(3) for s in range(2) for d in range(2)}
    ambiguous = {c for c in range(256) if _ambiguous_faces(c)}
    assert ambiguous <= seen_cubes                     # every cube index with an ambiguous face was exercised


def test_save_ply_round_trip(tmp_path):
    rs = np.random.RandomState(0)
    v = rs.randn(7, 3).astype(np.float32)
    n = rs.randn(7, 3).astype(np.float32)
    f = rs.randint(0, 7, size=(5, 3)).astype(np.int32)
    c = rs.randint(0, 256, size=(7, 3)).astype(np.uint8)
    for colors in (c, None):
        p = str(tmp_path / 'm.ply')
        mesh.save_ply(p, mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n),
                                   None if colors is None else torch.from_numpy(colors)))
        head, vert, faces = M.read_ply(p)
        assert 'element vertex 7' in head and 'element face 5' in head
        assert ('property uchar red' in head) == (colors is not None)
        np.testing.assert_array_equal(np.stack([vert['x'], vert['y'], vert['z']], -1), v)
        np.testing.assert_array_equal(np.stack([vert['nx'], vert['ny'], vert['nz']], -1), n)
        np.testing.assert_array_equal(faces, f)
        if colors is not None:
            np.testing.assert_array_equal(np.stack([vert['red'], vert['green'], vert['blue']], -1), c)


def test_frustum_bounds_are_the_frusta_corners():
    rs = np.random.RandomState(3)
    poses = []
    for _ in range(4):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        poses.append(np.concatenate([q, rs.randn(3, 1)], 1))
    poses = np.stack(poses).astype(np.float32)
    H, W, focal, near, far = 30, 40, 35.0, 0.5, 3.0
    corners = []
    for P in poses:
        for i, j in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            d = P[:3, :3].astype(np.float64) @ np.array([(i - W * 0.5) / focal, -(j - H * 0.5) / focal, -1.0])
            for z in (near, far):
                corners.append(P[:3, 3] + d * z)
    corners = np.array(corners)
    lo, hi = mesh.frustum_bounds(torch.from_numpy(poses), (H, W, focal), near, far)
    np.testing.assert_allclose(lo, corners.min(0), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(hi, corners.max(0), rtol=1e-6, atol=1e-6)


OK, EINVAL = 0, -1


def raw(name, *args):
    return getattr(_lib.load(), name)(*args)


def test_abi_argument_checks():
    lib = _lib.load()
    assert lib.mvip_mcubes_groups(64, 64, 64) == 256
    assert lib.mvip_mcubes_groups(2, 2, 2) == 1
    assert lib.mvip_mcubes_groups(1, 64, 64) == -1 and lib.mvip_mcubes_groups(769, 64, 64) == -1
    P = None
    # count: malformed (axis of 1 point, axis of 769, iso <= 0); well-formed shape with null operands.  No empty form.
    for bad in ((P, 1, 8, 8, 1.0, P, P, P, P, P), (P, 8, 769, 8, 1.0, P, P, P, P, P), (P, 8, 8, 8, 0.0, P, P, P, P, P),
                (P, 8, 8, 8, float('nan'), P, P, P, P, P)):
        assert raw('mvip_mcubes_count', *bad) == EINVAL
    assert raw('mvip_mcubes_count', P, 8, 8, 8, 1.0, P, P, P, P, P) == EINVAL
    box = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    # emit: malformed (bad axis, bmin >= bmax, negative count); empty (no vertices, no triangles); null operands
    assert raw('mvip_mcubes_emit', P, 8, 1, 8, 1.0, *box, P, P, P, 3, 1, P, P, P, P, P) == EINVAL
    assert raw('mvip_mcubes_emit', P, 8, 8, 8, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, P, P, P, 3, 1, P, P, P, P, P) == EINVAL
    assert raw('mvip_mcubes_emit', P, 8, 8, 8, 1.0, *box, P, P, P, -1, 1, P, P, P, P, P) == EINVAL
    assert raw('mvip_mcubes_emit', P, 8, 8, 8, 1.0, *box, P, P, P, 3, 2 ** 31, P, P, P, P, P) == EINVAL
    assert raw('mvip_mcubes_emit', P, 8, 8, 8, 1.0, *box, P, P, P, 0, 0, P, P, P, P, P) == OK
    assert raw('mvip_mcubes_emit', P, 8, 8, 8, 1.0, *box, P, P, P, 3, 1, P, P, P, P, P) == EINVAL


def test_python_argument_errors():
    g = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError):
        mesh.marching_cubes(g, 0.0, (0, 0, 0), (1, 1, 1))                 # threshold <= 0
    with pytest.raises(ValueError):
        mesh.marching_cubes(g, -1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        mesh.marching_cubes(g, 1.0, (0, 0, 0), (1, 0, 1))                 # bound_min >= bound_max on y
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 1, 4), 1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4), 1.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        mesh.grid_axes((0, 0, 0), (1, 1, 1), 769, 'cpu')
    with pytest.raises(ValueError):
        mesh.density_grid({'ndc': True, 'network_fn': None, 'network_query_fn': None}, (0, 0, 0), (1, 1, 1), 8)
    with pytest.raises(ValueError):
        mesh.frustum_bounds(np.eye(4)[:3], (4, 4, 2.0), 2.0, 1.0)
