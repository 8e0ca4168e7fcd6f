"""Mesh topology on the GPU (csrc/mesh_topology.hip) against its restatement tests/mesh_topology_numpy.py: every output tensor
of ops.mesh_edge_table / mesh_components / mesh_boundary_loops / mesh_cap_loops must be EQUAL to the restatement's -- integers,
and the bit patterns of the cap vertices -- on the marching-cubes meshes of tests/test_mesh_topology_cpu.py, the hand-made
meshes for every edge class, and three meshes built for the kernels' weak points: a strip of 4,096 triangles in scrambled face
order (deep union-find chains, one loop of 4,098 half-edges whose links cross workgroups), a fan of 300 triangles (lists longer
than a wave and than a workgroup), the cut sphere (3 F = 3,354: several compaction workgroups, the last one ragged).  Then
reproducibility, invariance under a permutation of the faces, mesh.topology / keep_components / close_holes, argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_topology_numpy as T                          # noqa: E402
from test_mesh_topology_cpu import TETRA                 # noqa: E402

from mvip_nerf_amd import mesh, ops                      # noqa: E402

pytestmark = pytest.mark.gpu


def _colors(n):
    return ((np.arange(3 * n, dtype=np.int64).reshape(n, 3) * 2654435761 >> 7) % 256).astype(np.uint8)


def _mc(case, *cut):
    v, f = T.mc_mesh(case)
    return v, (T.cut(v, f, *cut) if cut else f)


def _hand(faces, n_verts):
    rng = np.random.RandomState(n_verts)
    return rng.uniform(-1, 1, (n_verts, 3)).astype(np.float32), np.asarray(faces, np.int64).reshape(-1, 3)


def _flipped():
    f = TETRA.copy()
    f[2] = f[2, ::-1]
    return f


CASES = {
    'sphere': lambda: _mc('sphere24_3'),
    'cut_sphere': lambda: _mc('sphere24_3', 0, 0.2),
    'torus': lambda: _mc('torus32_6'),
    'cut_torus': lambda: _mc('torus32_6', 0, 0.0),
    'two_spheres': lambda: _mc('two_spheres24_2.5'),
    'cut_two_spheres': lambda: _mc('two_spheres24_2.5', 1, 0.25, True),
    'bow_tie': lambda: _hand([[0, 1, 2], [2, 3, 4]], 5),
    'fin': lambda: _hand([[0, 1, 2], [0, 1, 3], [1, 0, 4]], 5),
    'flipped': lambda: _hand(_flipped(), 4),
    'duplicated': lambda: _hand(np.concatenate([TETRA, TETRA[:1]]), 4),
    'degenerate': lambda: _hand([[0, 1, 2], [1, 1, 3], [2, 1, 3]], 4),
    'all_degenerate': lambda: _hand([[0, 0, 1], [2, 1, 2]], 3),
    'unreferenced': lambda: _hand(TETRA + 3, 9),
    'strip': T.strip,
    'fan': T.fan,
}
_made = {}


def get(name, cuda):
    """(verts, faces, colours) on the host and on the device, made once and left unchanged."""
    if name not in _made:
        v, f = CASES[name]()
        v, f, c = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), _colors(len(v))
        _made[name] = (v, f, c) + tuple(torch.tensor(x, device=cuda) for x in (v, f, c))
    return _made[name]


def same(got, want, what):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    else:
        assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, int(np.sum(got != want)), np.argwhere(got != want)[:5].tolist())


def test_the_meshes_have_the_shapes_the_kernels_can_go_wrong_at(cuda):
    f = get('cut_sphere', cuda)[1]
    assert 3 * len(f) == 3354 and 3 * len(f) > 3 * 1024 and (3 * len(f)) % 1024 != 0
    assert len(get('strip', cuda)[1]) == 4096 and np.bincount(get('fan', cuda)[1].reshape(-1))[0] == 300


@pytest.mark.parametrize('name', sorted(CASES))
def test_edge_table(name, cuda):
    v, f, _, _, fd, _ = get(name, cuda)
    got, want = ops.mesh_edge_table(fd, len(v)), T.edge_table(f, len(v))
    for field in want._fields:
        same(getattr(got, field), getattr(want, field), field)


@pytest.mark.parametrize('connectivity', ('edge', 'vertex'))
@pytest.mark.parametrize('name', sorted(CASES))
def test_components(name, connectivity, cuda):
    v, f, _, _, fd, _ = get(name, cuda)
    labels, table = ops.mesh_components(fd, len(v), connectivity)
    want = T.components(f, len(v), connectivity)
    same(labels, want[0], 'labels')
    same(table, want[1], 'table')


@pytest.mark.parametrize('name', sorted(CASES))
def test_boundary_loops(name, cuda):
    v, f, _, _, fd, _ = get(name, cuda)
    got, want = ops.mesh_boundary_loops(fd, len(v)), T.boundary_loops(f, len(v))
    for field in want._fields:
        same(getattr(got, field), getattr(want, field), field)


@pytest.mark.parametrize('name', sorted(CASES))
def test_cap_loops(name, cuda):
    v, f, c, vd, fd, cd = get(name, cuda)
    for max_edges, colors in ((64, True), (8192, False), (3, True)):
        got = ops.mesh_cap_loops(vd, fd, cd if colors else None, max_edges)
        want = T.cap_loops(v, f, c if colors else None, max_edges)
        same(got[0], want[0], 'new_verts')
        assert (got[1] is None) == (want[1] is None)
        if colors:
            same(got[1], want[1], 'new_colors')
        same(got[2], want[2], 'new_faces')
        same(got[3], want[3], 'capped')


def test_the_long_loop_is_refused_at_64_and_capped_at_8192(cuda):
    _, _, _, vd, fd, _ = get('strip', cuda)
    assert ops.mesh_boundary_loops(fd, vd.shape[0]).sizes.tolist() == [4098]
    nv, _, nf, capped = ops.mesh_cap_loops(vd, fd, None, 64)
    assert capped.tolist() == [0] and nv.shape == (0, 3) and nf.shape == (0, 3)
    nv, _, nf, capped = ops.mesh_cap_loops(vd, fd, None, 8192)
    assert capped.tolist() == [1] and nv.shape == (1, 3) and nf.shape == (4098, 3)


def test_twice_gives_the_same_bits(cuda):
    for name in ('strip', 'cut_two_spheres'):
        _, _, _, vd, fd, cd = get(name, cuda)
        V = vd.shape[0]
        runs = [tuple(ops.mesh_edge_table(fd, V)) + ops.mesh_components(fd, V) + ops.mesh_components(fd, V, 'vertex') +
                tuple(ops.mesh_boundary_loops(fd, V)) + ops.mesh_cap_loops(vd, fd, cd, 8192) for _ in range(2)]
        for a, b in zip(*runs):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize('name', ('cut_torus', 'cut_two_spheres'))
def test_permuted_faces_give_the_same_partition(name, cuda):
    v, f, _, _, fd, _ = get(name, cuda)
    perm = np.random.RandomState(5).permutation(len(f))                     # new face i = old face perm[i]
    pd = torch.from_numpy(perm).to(cuda)
    old_h = (3 * perm[:, None] + np.arange(3)).reshape(-1)                   # new half-edge -> old half-edge

    def bijection(new, old, n):
        pairs = {(int(a), int(b)) for a, b in zip(new, old)}
        return len(pairs) == n and len({a for a, _ in pairs}) == n and len({b for _, b in pairs}) == n

    labels, table = ops.mesh_components(fd, len(v))
    got, ptable = ops.mesh_components(fd[pd].contiguous(), len(v))
    got = got.cpu().numpy()
    assert bijection(got, labels.cpu().numpy()[perm], len(table)) and got[0] == 1          # numbered in the NEW order
    assert sorted(map(tuple, table.tolist())) == sorted(map(tuple, ptable.tolist()))
    loops, ploops = ops.mesh_boundary_loops(fd, len(v)), ops.mesh_boundary_loops(fd[pd].contiguous(), len(v))
    assert len(loops.first) == 2 and sorted(loops.sizes.tolist()) == sorted(ploops.sizes.tolist())
    assert bijection(ploops.loop_of.cpu().numpy(), loops.loop_of.cpu().numpy()[old_h], 3)  # two loops and "off the boundary"
    same(ploops.closed, loops.closed.cpu().numpy(), 'closed')


def _mesh(name, cuda, colors=True, normals=False):
    _, _, _, vd, fd, cd = get(name, cuda)
    return mesh.Mesh(vd, fd, ops.mesh_vertex_normals(vd, fd) if normals else None, cd if colors else None)


def test_keep_components(cuda):
    m = _mesh('two_spheres', cuda)
    v, f, c = get('two_spheres', cuda)[:3]
    labels, table = T.components(f, len(v))
    big = int(np.argmax(table[:, 0])) + 1
    assert table[0, 0] != table[1, 0]
    out = mesh.keep_components(m, largest=1)
    used = np.zeros(len(v), bool)
    used[f[labels == big].reshape(-1)] = True
    new = np.cumsum(used) - 1
    same(out.verts, v[used], 'verts')
    same(out.colors, c[used], 'colors')
    same(out.faces, new[f[labels == big]].astype(np.int32), 'faces')
    small = 3 - big
    p = v[f[labels == small][0]].astype(np.float64).mean(0) * 1.01           # just off a face of the smaller sphere
    both = mesh.keep_components(m, largest=1, containing=p[None])
    same(both.faces, f, 'faces')
    same(both.verts, v, 'verts')
    only = mesh.keep_components(m, containing=torch.tensor(p[None], dtype=torch.float32))
    assert only.faces.shape[0] == table[small - 1, 0]
    assert mesh.keep_components(m, min_faces=int(table[:, 0].max())).faces.shape[0] == table[:, 0].max()
    with pytest.raises(ValueError):
        mesh.keep_components(m)
    with pytest.raises(ValueError):
        mesh.keep_components(m, largest=0)


def test_close_holes_and_topology(cuda):
    m = _mesh('cut_sphere', cuda, normals=True)
    V, F = m.verts.shape[0], m.faces.shape[0]
    rep = mesh.topology(m)
    assert (rep['vertices'], rep['faces'], rep['edges'], rep['euler'], rep['genus']) == (580, 1118, 1697, 1, None)
    assert rep['loops'] == 1 and rep['closed_loops'] == 1 and not rep['closed'] and rep['oriented']
    out, capped, left = mesh.close_holes(m)
    assert (capped, left) == (1, 0) and out.verts.shape[0] == V + 1 and out.faces.shape[0] == F + 40
    for old, new in ((m.verts, out.verts), (m.normals, out.normals)):
        assert torch.equal(old.view(torch.int32), new[:V].view(torch.int32))
    assert torch.equal(m.faces, out.faces[:F]) and torch.equal(m.colors, out.colors[:V])
    assert torch.equal(out.normals[V:].view(torch.int32), ops.mesh_vertex_normals(out.verts, out.faces)[V:].view(torch.int32))
    rep = mesh.topology(out)
    assert rep['closed'] and rep['oriented'] and rep['genus'] == 0 and rep['euler'] == 2 and rep['components'] == 1
    assert rep['per_component'][0]['faces'] == F + 40 and rep['loops'] == 0
    same_mesh, capped, left = mesh.close_holes(m, max_edges=39)
    assert same_mesh is m and (capped, left) == (0, 1)
    loops = mesh.boundary_loops(m)
    assert loops.sizes.tolist() == [40]
    torus = mesh.topology(_mesh('torus', cuda))
    assert torus['genus'] == 1 and torus['euler'] == 0
    two = mesh.topology(_mesh('two_spheres', cuda), 'vertex')
    assert two['components'] == 2 and two['euler'] == 4 and two['genus'] == 0
    assert mesh.topology(_mesh('flipped', cuda))['genus'] is None
    assert mesh.topology(_mesh('degenerate', cuda))['degenerate_faces'] == 1


def test_empty_meshes_launch_nothing(cuda):
    f0 = torch.zeros((0, 3), device=cuda, dtype=torch.int32)
    et = ops.mesh_edge_table(f0, 7)
    assert et.edges.shape == (0, 2) and all(t.numel() == 0 and t.dtype == torch.int32 for t in et)
    labels, table = ops.mesh_components(f0, 0)
    assert labels.shape == (0,) and table.shape == (0, 6)
    assert all(t.shape == (0,) for t in ops.mesh_boundary_loops(f0, 7))
    v = torch.zeros((7, 3), device=cuda)
    nv, nc, nf, capped = ops.mesh_cap_loops(v, f0, torch.zeros((7, 3), device=cuda, dtype=torch.uint8), 64)
    assert nv.shape == (0, 3) and nc.shape == (0, 3) and nf.shape == (0, 3) and capped.shape == (0,)
    rep = mesh.topology(mesh.Mesh(v, f0, None, None))
    assert rep['components'] == 0 and rep['euler'] == 0 and rep['closed'] and rep['genus'] == 0


def test_argument_checks(cuda):
    _, _, _, vd, fd, cd = get('fin', cuda)
    V = vd.shape[0]
    for fn in (ops.mesh_edge_table, ops.mesh_components, ops.mesh_boundary_loops):
        for bad in (fd.cpu(), fd.to(torch.int64), fd.reshape(-1), fd.t(), fd.tolist()):
            with pytest.raises(ValueError):
                fn(bad, V)
        with pytest.raises(ValueError):
            fn(fd, V - 1)                                                    # index 4 outside [0, 4)
        with pytest.raises(ValueError):
            fn(fd, 0)
        with pytest.raises(ValueError):
            fn(fd, -1)
        with pytest.raises(ValueError):
            fn(torch.tensor([[0, 1, -1]], device=cuda, dtype=torch.int32), V)
    for connectivity in ('face', 6, None):
        with pytest.raises(ValueError):
            ops.mesh_components(fd, V, connectivity)
    for max_edges in (2, 0, -1, 3.5):
        with pytest.raises(ValueError):
            ops.mesh_cap_loops(vd, fd, cd, max_edges)
    for args in ((vd.double(), fd, cd), (vd, fd, cd[:-1]), (vd, fd, cd.to(torch.int32)), (vd.cpu(), fd, cd), (vd[:-1], fd, None)):
        with pytest.raises(ValueError):
            ops.mesh_cap_loops(*args, 64)
