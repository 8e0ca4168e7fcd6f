"""The restatement of the mesh topology (tests/mesh_topology_numpy.py) against first principles, on the CPU: the Euler
characteristics of a sphere, a torus and two spheres, the loops a planar cut leaves and what capping them does, and hand-made
meshes for every edge class.  tests/test_mesh_topology.py then checks the HIP kernels against the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ops_numpy as R                               # noqa: E402
import mesh_topology_numpy as T                          # noqa: E402

TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)     # closed, consistently oriented


def capped(v, f, max_edges=64):
    nv, _, nf, cap = T.cap_loops(v, f, None, max_edges)
    return np.concatenate([v, nv]), np.concatenate([f, nf.astype(np.int64)]), cap


def test_sphere():
    v, f = T.mc_mesh('sphere24_3')
    r = T.report(f, len(v))
    assert (len(v), r['vertices'], r['faces'], r['edges'], r['euler']) == (888, 888, 1772, 2658, 2)
    assert r['components'] == 1 and r['boundary_edges'] == 0 and r['closed'] and r['oriented'] and r['genus'] == 0
    et = T.edge_table(f, len(v))
    assert np.all(et.count == 2) and np.all(et.forward == 1) and np.all(et.twin >= 0)
    assert np.array_equal(et.twin[et.twin], np.arange(3 * len(f)))
    assert np.all(np.diff(et.first) > 0) and np.array_equal(et.edge_of[et.first], np.arange(len(et.first)))


def test_cut_sphere_and_its_cap():
    v, f = T.mc_mesh('sphere24_3')
    f = T.cut(v, f, 0, 0.2)
    r = T.report(f, len(v))
    assert (r['vertices'], r['faces'], r['edges'], r['euler']) == (580, 1118, 1697, 1)
    assert r['components'] == 1 and r['loops'] == 1 and r['closed_loops'] == 1 and r['genus'] is None
    lp = T.boundary_loops(f, len(v))
    assert lp.sizes.tolist() == [40] and np.all(lp.next[lp.loop_of >= 0] >= 0)          # no pinch vertex
    h, seen = int(lp.first[0]), []
    for _ in range(40):                                                                  # next walks one simple cycle
        seen.append(h)
        h = int(lp.next[h])
    assert h == lp.first[0] and len(set(seen)) == 40
    a, b, _ = T.half_edges(f)
    assert all(b[s] == a[lp.next[s]] for s in seen)
    v2, f2, cap = capped(v, f)
    assert cap.tolist() == [1] and len(v2) == len(v) + 1 and len(f2) == len(f) + 40
    r2 = T.report(f2, len(v2))
    assert r2['euler'] == 2 and r2['boundary_edges'] == 0 and r2['genus'] == 0
    assert R.directed_edge_balance(f2) == 0
    ring = v[a[np.nonzero(lp.loop_of == 0)[0]]].astype(np.float64)
    assert np.allclose(v2[-1], ring.mean(0), atol=1e-6)
    assert capped(v, f, max_edges=39)[2].tolist() == [0]


def test_torus():
    v, f = T.mc_mesh('torus32_6')
    r = T.report(f, len(v))
    assert (r['vertices'], r['faces'], r['edges'], r['euler'], r['genus']) == (1920, 3840, 5760, 0, 1)
    f = T.cut(v, f, 0, 0.0)
    lp = T.boundary_loops(f, len(v))
    assert len(f) == 1860 and lp.sizes.tolist() == [30, 30] and lp.closed.tolist() == [1, 1]
    v2, f2, _ = capped(v, f)
    r2 = T.report(f2, len(v2))
    assert r2['euler'] == 2 and r2['closed'] and r2['oriented'] and R.directed_edge_balance(f2) == 0


def test_two_spheres():
    v, f = T.mc_mesh('two_spheres24_2.5')
    labels, table = T.components(f, len(v))
    assert len(table) == 2 and T.report(f, len(v))['euler'] == 4
    assert np.all(table[:, 1] - table[:, 2] + table[:, 0] == 2)
    assert labels[0] == 1 and np.all(np.diff([np.nonzero(labels == c)[0][0] for c in (1, 2)]) > 0)
    assert np.array_equal(T.components(f, len(v), 'vertex')[0], labels)
    f = T.cut(v, f, 1, 0.25, absolute=True)
    lp = T.boundary_loops(f, len(v))
    assert len(T.components(f, len(v))[1]) == 2 and sorted(lp.sizes.tolist()) == [28, 31] and lp.closed.tolist() == [1, 1]


def test_bow_tie():
    f = np.array([[0, 1, 2], [2, 3, 4]])
    assert T.components(f, 5)[0].tolist() == [1, 2] and T.components(f, 5, 'vertex')[0].tolist() == [1, 1]
    assert T.components(f, 5, 'vertex')[1].tolist() == [[2, 5, 6, 6, 0, 0]]
    lp = T.boundary_loops(f, 5)
    assert np.all(lp.loop_of >= 0) and not lp.closed.any()              # two start and two end at the shared vertex
    assert lp.next.tolist() == [1, -1, 0, 4, 5, -1] and lp.sizes.tolist() == [3, 3]
    assert T.cap_loops(np.zeros((5, 3), np.float32), f, None, 64)[3].tolist() == [0, 0]


def test_fin():
    f = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]])
    et = T.edge_table(f, 5)
    e = et.edge_of[0]
    assert et.edges[e].tolist() == [0, 1] and et.count[e] == 3 and et.forward[e] == 2 and et.twin[0] == -1
    assert T.components(f, 5)[1].tolist() == [[3, 5, 7, 6, 1, 0]]
    r = T.report(f, 5)
    assert not r['closed'] and not r['oriented'] and r['genus'] is None


def test_flipped_face():
    assert T.report(TETRA, 4)['genus'] == 0
    f = TETRA.copy()
    f[2] = f[2, ::-1]
    r = T.report(f, 4)
    assert r['inconsistent_edges'] == 3 and r['closed'] and not r['oriented'] and r['genus'] is None
    et = T.edge_table(f, 4)
    assert sorted(et.forward[et.forward != 1].tolist()) in ([0, 0, 2], [0, 2, 2])


def test_duplicated_face():
    f = np.concatenate([TETRA, TETRA[:1]])
    et = T.edge_table(f, 4)
    assert sorted(et.count.tolist()) == [2, 2, 2, 3, 3, 3] and T.report(f, 4)['non_manifold_edges'] == 3
    assert T.components(f, 4)[0].tolist() == [1] * 5


def test_degenerate_face():
    f = np.array([[0, 1, 2], [1, 1, 3], [2, 1, 3]])
    et = T.edge_table(f, 4)
    assert et.edge_of[3:6].tolist() == [-1, -1, -1] and et.twin[3:6].tolist() == [-1, -1, -1]
    labels, table = T.components(f, 4)
    assert labels.tolist() == [1, 0, 1] and table.tolist() == [[2, 4, 5, 4, 0, 0]]
    assert np.all(T.boundary_loops(f, 4).loop_of[3:6] == -1)
    assert T.components(f, 4, 'vertex')[0].tolist() == [1, 0, 1]


def test_unreferenced_vertices_and_the_empty_mesh():
    assert T.components(TETRA + 3, 9)[1].tolist() == [[4, 4, 6, 0, 0, 0]]
    empty = np.zeros((0, 3), np.int64)
    et = T.edge_table(empty, 5)
    assert all(len(x) == 0 for x in et) and et.edges.shape == (0, 2)
    labels, table = T.components(empty, 5)
    assert labels.shape == (0,) and table.shape == (0, 6)
    assert all(len(x) == 0 for x in T.boundary_loops(empty, 5))
    nv, nc, nf, cap = T.cap_loops(np.zeros((5, 3), np.float32), empty, np.zeros((5, 3), np.uint8), 64)
    assert nv.shape == (0, 3) and nc.shape == (0, 3) and nf.shape == (0, 3) and cap.shape == (0,)
    with pytest.raises(ValueError):
        T.edge_table(TETRA, 3)


def test_strip_and_fan():
    v, f = T.strip()
    r = T.report(f, len(v))
    assert (r['components'], r['euler'], r['loops'], r['closed_loops'], r['boundary_edges']) == (1, 1, 1, 1, 4098)
    assert T.cap_loops(v, f, None, 64)[3].tolist() == [0] and T.cap_loops(v, f, None, 8192)[3].tolist() == [1]
    v, f = T.fan()
    assert np.bincount(f.reshape(-1))[0] == 300 and T.boundary_loops(f, len(v)).sizes.tolist() == [300]


def test_colour_mean_is_the_integer_formula():
    v, f = T.fan(5)
    col = np.array([[9, 9, 9], [1, 0, 255], [2, 0, 255], [2, 1, 255], [2, 0, 254], [2, 0, 255]], np.uint8)
    assert T.cap_loops(v, f, col, 64)[1].tolist() == [[2, 0, 255]]           # 9 / 5 -> 2, 1 / 5 -> 0, 1274 / 5 -> 255
