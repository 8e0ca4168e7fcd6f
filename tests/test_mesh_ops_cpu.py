"""The restatement of the mesh clean-up (tests/mesh_ops_numpy.py) against first principles, on the CPU: the corner table is a
grouped permutation, face normals of a sphere point radially, the umbrella vanishes on a flat regular grid, Taubin keeps the
volume that plain Laplacian smoothing loses, clustering keeps closed meshes closed and every representative in its cell,
dedupe removes exactly the repeated cycles, colour means are the exact integer formula.  tests/test_mesh_ops.py then checks
the HIP kernels against the restatement."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402


@functools.lru_cache(maxsize=None)
def mesh_of(npts, fn):
    v, f, n = M.marching_cubes(R.lattice(npts, fn), 1.0, R.LO, R.HI)
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


def sphere24():
    return mesh_of(24, R.CLUSTER_CASES[0][2])


def cut_open(v, f):
    """the faces with all three vertices at x < 0.2: a boundary loop, and the vertices beyond it unreferenced."""
    return f[np.all(v[f][:, :, 0] < 0.2, axis=1)]


def angle_deg(a, b):
    return np.degrees(np.arccos(np.clip(np.einsum('ij,ij->i', a.astype(np.float64), b.astype(np.float64)), -1.0, 1.0)))


def test_corner_table_is_a_grouped_ascending_permutation():
    v, f, _ = sphere24()
    for faces, V in ((f, len(v)), (cut_open(v, f), len(v)), (np.zeros((0, 3), np.int64), 5)):
        off, cor = R.corner_table(faces, V)
        assert off.shape == (V + 1,) and off[0] == 0 and off[-1] == 3 * len(faces)
        assert np.array_equal(np.sort(cor), np.arange(3 * len(faces)))
        flat = np.asarray(faces).reshape(-1)
        for u in range(V):
            mine = cor[off[u]:off[u + 1]]
            assert np.all(flat[mine] == u) and np.all(np.diff(mine) > 0)
    assert 3 * len(f) > 1024 and (3 * len(f)) % 1024 != 0          # more than one workgroup of the compaction, and a ragged one
    assert np.any(np.diff(R.corner_table(cut_open(v, f), len(v))[0]) == 0)   # the cut leaves unreferenced vertices


def test_sphere_normals_point_radially():
    """Face normals of the 24^3 sphere (radius 0.6, 888 vertices): the largest angle to the analytic radial direction is
    5.87 degrees, to the lattice normals of marching cubes 5.88 degrees (those are within 0.22 degrees of radial): the
    area-weighted sum sees the sliver triangles marching cubes leaves where the surface passes close to a lattice point.
    Bound 6.0 degrees: the computation is fp64 and deterministic, the margin of 2 % only covers another libm's arccos / sqrt
    and a marching-cubes vertex moving by an fp32 ulp."""
    v, f, lattice_normals = sphere24()
    n = R.vertex_normals(v, f)
    assert n.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    to_radial, to_lattice = angle_deg(n, radial).max(), angle_deg(n, lattice_normals).max()
    print(f'largest angle: to radial {to_radial:.3f} deg, to the lattice normals {to_lattice:.3f} deg')
    assert to_radial <= 6.0 and to_lattice <= 6.0
    assert np.all(np.einsum('ij,ij->i', n, v) > 0)                  # outward
    # unreferenced vertices and the boundary
    fc = cut_open(v, f)
    nc = R.vertex_normals(v, fc)
    lone = np.bincount(fc.reshape(-1), minlength=len(v)) == 0
    assert lone.any() and np.all(nc[lone] == 0) and np.all(np.linalg.norm(nc[~lone], axis=1) > 0.999)


def rounding_gap_normals(v, f):
    return float(np.abs(R.vertex_normals(v, f, 'fp64') - R.vertex_normals(v, f, 'fp32')).max())


def rounding_gap_smooth(v, f, iters):
    return float(np.abs(R.smooth(v, f, iters, rounding='fp64') - R.smooth(v, f, iters, rounding='fp32')).max())


def test_rounding_gaps_are_fp32_rounding():
    """d of the GPU comparison: the restatement in fp64 against the restatement with fp32 rounding at the kernel's rounding
    points.  On the 24^3 sphere: normals d = 3.0e-8 (half an fp32 ulp of a component below 1), 10 Taubin iterations
    d = 1.8e-7 (20 roundings of coordinates below 1, each at most 3e-8, partly cancelling)."""
    v, f, _ = sphere24()
    dn, ds = rounding_gap_normals(v, f), rounding_gap_smooth(v, f, 10)
    print(f'd: normals {dn:.3e}, smoothing {ds:.3e}')
    assert 0 < dn <= 2.0 ** -24 and 0 < ds <= 20 * 2.0 ** -24


def test_umbrella_vanishes_on_a_flat_regular_grid():
    n = 9
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = np.stack([i * 0.125, j * 0.25, np.full_like(i, 0.5, dtype=np.float64)], -1).reshape(-1, 3).astype(np.float32)
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([q, q + n, q + n + 1], -1), np.stack([q, q + n + 1, q + 1], -1)])
    out = R.smooth_pass(v.astype(np.float64), f, 0.5)
    interior = ((i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)).reshape(-1)
    np.testing.assert_allclose(out[interior], v[interior], rtol=0, atol=1e-15)
    assert np.abs(out[~interior] - v[~interior]).max() > 1e-3       # the border does move: its umbrella is one-sided


def test_taubin_keeps_the_volume_plain_laplacian_loses():
    v, f, _ = sphere24()
    noisy = (v + np.random.RandomState(0).normal(0, 0.01, v.shape)).astype(np.float32)
    taubin = R.smooth(noisy, f, 10, 0.5, -0.53, rounding='fp64')
    plain = noisy.astype(np.float64)
    for _ in range(10):
        plain = R.smooth_pass(plain, f, 0.5)
    radial_rms = lambda p: float(np.std(np.linalg.norm(p, axis=1)))
    assert radial_rms(taubin) < radial_rms(noisy) and radial_rms(plain) < radial_rms(noisy)
    vol = M.signed_volume(noisy, f)
    assert abs(M.signed_volume(taubin, f) - vol) < abs(M.signed_volume(plain, f) - vol)
    # vertices without faces stay where they are
    fc = cut_open(v, f)
    lone = np.bincount(fc.reshape(-1), minlength=len(v)) == 0
    assert np.array_equal(R.smooth(noisy, fc, 3)[lone], noisy[lone])


def cluster_case(name, placement='quadric', dedupe=False, colors=False):
    _, npts, fn, steps, origin = next(c for c in R.CLUSTER_CASES if c[0] == name)
    v, f, _ = mesh_of(npts, fn)
    col = np.random.RandomState(3).randint(0, 256, v.shape).astype(np.uint8) if colors else None
    return v, f, col, R.cluster(v, f, col, None if origin is None else R.LO, steps * R.step(npts), placement, dedupe)


@pytest.mark.parametrize('name', [c[0] for c in R.CLUSTER_CASES])
@pytest.mark.parametrize('placement', ('mean', 'quadric'))
def test_clustering_keeps_closed_meshes_closed(name, placement):
    v, f, _, res = cluster_case(name, placement)
    assert R.directed_edge_balance(f) == 0                          # the input is closed
    fo, vo = res['faces'], res['verts']
    assert 0 < len(fo) < len(f) / 3 and len(vo) < len(v) / 3
    assert R.directed_edge_balance(fo) == 0                         # exactly
    assert np.all((fo[:, 0] != fo[:, 1]) & (fo[:, 1] != fo[:, 2]) & (fo[:, 0] != fo[:, 2]))
    assert np.array_equal(np.unique(fo), np.arange(len(vo)))        # every vertex referenced
    assert np.array_equal(R.cell_of(vo, res['origin'], res['inv'], res['cells']), res['cell_of_cluster'])
    assert np.all(np.diff(res['cell_of_cluster']) > 0)              # ids ascend in cell order
    cov = res['cluster_of_vertex']
    assert np.array_equal(R.cell_of(v, res['origin'], res['inv'], res['cells'])[cov >= 0], res['cell_of_cluster'][cov[cov >= 0]])
    cell = next(c[3] for c in R.CLUSTER_CASES if c[0] == name) * R.step(next(c[1] for c in R.CLUSTER_CASES if c[0] == name))
    assert np.linalg.norm(vo[cov[cov >= 0]].astype(np.float64) - v[cov >= 0], axis=1).max() <= np.sqrt(3.0) * cell * (1 + 1e-6)
    if placement == 'quadric':
        assert res['used_quadric'].mean() > 0.5                     # the quadric is what places most clusters


def test_on_face_case_has_vertices_on_cell_faces_and_long_lists_exist():
    v, f, _, res = cluster_case('sphere24_2box')
    t = (v.astype(np.float64) - res['origin']) / (2.0 * R.step(24))
    assert np.mean(np.any(np.abs(t - np.round(t)) < 1e-6, axis=1)) > 0.5
    v, f, _, res = cluster_case('torus32_6')
    assert np.bincount(res['cluster_of_vertex'][f.reshape(-1)]).max() > 64


@pytest.mark.parametrize('name', R.QUADRIC_CASES)
def test_borderline_quadric_clusters_stay_under_the_cap(name):
    _, _, _, res = cluster_case(name)
    assert R.borderline(res).mean() <= R.MAX_SKIPPED_SHARE


def with_repeats(f):
    """the faces, then every 7th again rotated by one, then every 11th again with the opposite orientation (a different face)."""
    return np.concatenate([f, np.roll(f[::7], 1, axis=1), f[::11][:, ::-1]])


def test_dedupe_removes_exactly_the_repeated_cycles():
    v, f, _ = sphere24()
    ff = with_repeats(f)
    cell = 0.25 * R.step(24)                                        # small cells: most faces survive, a few slivers collapse
    res = R.cluster(v, ff, None, None, cell, 'mean', dedupe=True)
    plain = R.cluster(v, ff, None, None, cell, 'mean', dedupe=False)
    cov = plain['cluster_of_vertex']
    assert np.array_equal(cov, res['cluster_of_vertex'])
    seen, expect = set(), []
    for a, b, c in cov[ff]:
        if a == b or b == c or a == c:
            continue
        k = min((a, b, c), (b, c, a), (c, a, b))
        if k not in seen:
            seen.add(k)
            expect.append((a, b, c))
    assert np.array_equal(res['faces'], np.asarray(expect, np.int32))
    r7 = cov[f[::7]]
    alive = (r7[:, 0] != r7[:, 1]) & (r7[:, 1] != r7[:, 2]) & (r7[:, 0] != r7[:, 2])
    assert alive.sum() > 100 and len(plain['faces']) - len(res['faces']) == alive.sum()   # the rotated repeats go, the reversed copies stay
    assert R.directed_edge_balance(plain['faces']) != 0             # (this input was not closed: the repeats unbalance it)


def test_colour_means_are_the_integer_formula():
    v, f, col, res = cluster_case('sphere24_3', 'mean', colors=True)
    cov = res['cluster_of_vertex']
    assert res['colors'].dtype == np.uint8 and res['colors'].shape == res['verts'].shape
    for k in range(len(res['verts'])):
        members = col[cov == k].astype(int)
        n = len(members)
        for t in range(3):
            s = int(members[:, t].sum())
            assert res['colors'][k, t] == (2 * s + n) // (2 * n)
            assert abs(int(res['colors'][k, t]) - s / n) <= 0.5


def test_mean_placement_is_the_mean():
    v, f, _, res = cluster_case('two_spheres24_2.5', 'mean')
    cov = res['cluster_of_vertex']
    for k in range(0, len(res['verts']), 5):
        np.testing.assert_allclose(res['verts'][k], v[cov == k].astype(np.float64).mean(0), rtol=0, atol=2e-7)


def test_quadric_minimiser_solves_the_normal_equations():
    """On a cluster the quadric places, x minimises sum (N . x + d)^2: checked by the gradient, rebuilt here from the faces."""
    v, f, _, res = cluster_case('torus32_6')
    cov = res['cluster_of_vertex']
    cell = 6.0 * R.step(32)
    p = v.astype(np.float64)
    checked = 0
    for k in np.nonzero(res['used_quadric'] & ~R.borderline(res))[0][:8]:
        A, B = np.zeros((3, 3)), np.zeros(3)
        for face in f:
            times = int(np.sum(cov[face] == k))                     # a face with two corners in the cluster counts twice
            if times:
                N = np.cross(p[face[1]] - p[face[0]], p[face[2]] - p[face[0]])
                A += times * np.outer(N, N)
                B += times * (-(N @ p[face[0]])) * N
        x = res['verts'][k].astype(np.float64)
        # x is rounded to fp32: A x is off by up to |A| |x| 2^-24, |x| < 1 < 3 cell
        assert np.linalg.norm(A @ x + B) <= 1e-6 * np.linalg.norm(A) * cell
        checked += 1
    assert checked > 0
