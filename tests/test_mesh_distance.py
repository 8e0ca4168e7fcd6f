"""Mesh-to-mesh distance on the GPU (csrc/mesh_distance.hip) against its brute-force restatement tests/mesh_distance_numpy.py:
closest-point queries on the face grid (face, point and dist BIT-EQUAL: the result must not depend on the grid), the grid's
lists, surface samples, evaluate.mesh_distance_metrics, the argument checks of ops and of the C ABI, tools/extract_mesh.py
--report-error.  The meshes are what mesh.marching_cubes makes of the analytic lattices of tests/mesh_ops_numpy.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402

from mvip_nerf_amd import _lib, evaluate, mesh, ops      # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
_meshes, _refs = {}, {}


def big_sphere(x, y, z):
    return R.sphere_field(0.9)(x, y, z)


MESHES = {
    'sphere24': (24, R.CLUSTER_CASES[0][2], False),
    'cut24': (24, R.CLUSTER_CASES[0][2], True),            # the cut-open sphere: a boundary loop, and a vertex no face references
    'two_spheres24': (24, R.two_spheres_field, False),     # a non-cubic bounding box
    'torus32': (32, R.torus_field, False),
    'sphere136': (136, big_sphere, False),                 # V above 65,536, about 1.4e5 faces
}


def get(name, cuda):
    """(verts, faces) device tensors and their numpy copies, made once."""
    if name not in _meshes:
        npts, fn, cut = MESHES[name]
        grid = torch.from_numpy(R.lattice(npts, fn)).to(cuda)
        valid = None
        if cut:
            ax = F32(R.LO[0]) + np.arange(npts, dtype=F32) * F32(R.step(npts))
            valid = torch.from_numpy(np.broadcast_to((ax < 0.2)[:, None, None], (npts,) * 3).copy()).to(cuda)
        v, f, _ = mesh.marching_cubes(grid, 1.0, R.LO, R.HI, valid=valid)
        if cut:
            v = torch.cat([v, torch.tensor([[0.9, 0.9, 0.9]], device=cuda)]).contiguous()
        vn, fn_ = v.cpu().numpy(), f.cpu().numpy()
        vn.setflags(write=False)
        fn_.setflags(write=False)
        _meshes[name] = (v, f, vn, fn_)
    return _meshes[name]


def cluster_samples(name, cuda):
    """the samples (device, numpy) of the mesh clustered at 3 lattice steps: 9 per face (4 on the torus, which has the most faces)"""
    v, f, _, _ = get(name, cuda)
    cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, 3 * R.step(MESHES[name][0]))
    pts = ops.mesh_sample_faces(cv, cf, 2 if name == 'torus32' else 3)[0]
    return pts, pts.cpu().numpy()


def reference(key, pts, vn, fn):
    """the brute-force answer for a query set, computed once and left unchanged"""
    if key not in _refs:
        out = D.closest_point(pts, vn, fn, chunk=1 << 21)
        for a in out:
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def same(got, ref, what=''):
    face, point, dist = (t.cpu().numpy() for t in got[:3])
    assert face.dtype == I32 and point.dtype == F32 and dist.dtype == F32
    np.testing.assert_array_equal(face, ref[0], err_msg=what + ' face')
    np.testing.assert_array_equal(dist, ref[2], err_msg=what + ' dist')       # NaN == NaN here
    np.testing.assert_array_equal(point, ref[1], err_msg=what + ' point')


@pytest.mark.parametrize('name', ['sphere24', 'cut24', 'two_spheres24', 'torus32'])
def test_samples_of_the_clustered_mesh_equal_brute_force(name, cuda):
    v, f, vn, fn = get(name, cuda)
    pts, pn = cluster_samples(name, cuda)
    assert len(pn) > 512 and len(pn) * len(fn) <= 5e7                                 # several workgroups
    assert name != 'sphere24' or (len(pn) > 1025 and len(pn) % 256 != 0)               # and a ragged last one
    ref = reference((name, 'cluster'), pn, vn, fn)
    assert ref[2].max() > 0
    same(ops.mesh_closest_point(pts, v, f), ref, name)
    grid = ops.mesh_face_grid(v, f)                                                 # a grid reused, and given explicitly
    same(ops.mesh_closest_point(pts, v, f, grid=grid), ref, name)
    same(ops.mesh_closest_point(pts, v, f, grid=grid), ref, name)


@pytest.mark.parametrize('name', ['sphere24', 'cut24'])
def test_own_vertices_are_at_distance_zero_on_their_lowest_face(name, cuda):
    v, f, vn, fn = get(name, cuda)
    face, point, dist = ops.mesh_closest_point(v, v, f)
    same((face, point, dist), reference((name, 'vertices'), vn, vn, fn), name)
    lowest = np.full(len(vn), len(fn), np.int64)                                       # the lowest face index at every vertex
    np.minimum.at(lowest, fn.reshape(-1), np.repeat(np.arange(len(fn)), 3))
    used = lowest < len(fn)
    assert used.sum() >= len(vn) - 1 and (name != 'cut24' or not used[-1])
    assert np.all(dist.cpu().numpy()[used] == 0)
    np.testing.assert_array_equal(face.cpu().numpy()[used], lowest[used])               # the tie rule: several faces at distance 0
    np.testing.assert_array_equal(point.cpu().numpy()[used], vn[used])


def test_points_far_outside_the_box_walk_the_whole_grid(cuda):
    v, f, vn, fn = get('two_spheres24', cuda)
    rng = np.random.default_rng(11)
    d = rng.standard_normal((90, 3))
    far = np.concatenate([50.0 * d / np.linalg.norm(d, axis=1, keepdims=True),
                          [[1e6, 0, 0], [0, -1e6, 0], [0.1, 0.1, 3e8], [-40, -40, -40], [2, 0, 0], [0, 0, -1.5]]]).astype(F32)
    grid = ops.mesh_face_grid(v, f)
    got = ops.mesh_closest_point(torch.from_numpy(far).to(cuda), v, f, grid=grid, return_stats=True)
    same(got, reference(('two_spheres24', 'far'), far, vn, fn))
    assert int(got[3].cpu()[0]) >= grid.n_pairs                                           # at least one query met every list


def _on_plane(o, inv, k):
    """an fp32 x with (x - o) * inv == k exactly in fp32 arithmetic, or None"""
    x = F32(o) + F32(k) / F32(inv)
    for cand in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
        cand = F32(cand)
        if F32(F32(cand - F32(o)) * F32(inv)) == F32(k):
            return cand
    return None


def test_points_exactly_on_cell_planes(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    grid = ops.mesh_face_grid(v, f, cells=(8, 5, 4))
    assert grid.cells == (8, 5, 4)
    planes = [[x for x in (_on_plane(grid.box[a], grid.box[3 + a], k) for k in range(grid.cells[a] + 1)) if x is not None] for a in range(3)]
    assert all(len(p) >= 3 for p in planes), planes
    rng = np.random.default_rng(5)
    lo, hi = vn.min(0), vn.max(0)
    pts = []
    for a in range(3):
        for x in planes[a]:
            p = rng.uniform(lo, hi, (6, 3)).astype(F32)
            p[:, a] = x
            pts.append(p)
    pts.append(np.asarray([[x, y, z] for x in planes[0][:3] for y in planes[1][:3] for z in planes[2][:3]], F32))     # corners of cells
    pts = np.concatenate(pts)
    ref = reference(('sphere24', 'planes'), pts, vn, fn)
    same(ops.mesh_closest_point(torch.from_numpy(pts).to(cuda), v, f, grid=grid), ref)
    same(ops.mesh_closest_point(torch.from_numpy(pts).to(cuda), v, f), ref)


@pytest.mark.parametrize('n', [1, 1025])
def test_query_arrays_of_length_one_and_1025(n, cuda):
    v, f, vn, fn = get('sphere24', cuda)
    pts, pn = cluster_samples('sphere24', cuda)
    ref = reference(('sphere24', 'cluster'), pn, vn, fn)
    same(ops.mesh_closest_point(pts[:n].contiguous(), v, f), tuple(r[:n] for r in ref))
    same(ops.mesh_closest_point(pts[-n:].contiguous(), v, f), tuple(r[-n:] for r in ref))
    empty = ops.mesh_closest_point(pts[:0].contiguous(), v, f)
    assert [tuple(t.shape) for t in empty] == [(0,), (0, 3), (0,)]


def test_result_does_not_depend_on_the_grid(cuda):
    v, f, vn, fn = get('two_spheres24', cuda)                                         # a non-cubic box
    assert np.ptp(vn, axis=0).max() > 1.5 * np.ptp(vn, axis=0).min()
    pts, pn = cluster_samples('two_spheres24', cuda)
    ref = reference(('two_spheres24', 'cluster'), pn, vn, fn)
    tests = {}
    for cells in (1, 2, 7, None):
        grid = ops.mesh_face_grid(v, f, cells=cells)
        got = ops.mesh_closest_point(pts, v, f, grid=grid, return_stats=True)
        same(got, ref, f'cells={cells}')
        tests[cells], slots = (int(x) for x in got[3].cpu())
        assert tests[cells] <= slots <= 64 * tests[cells]
    print('point-face tests per query:', {k: t / len(pn) for k, t in tests.items()}, 'faces', len(fn))
    assert tests[1] == len(pn) * len(fn)                                               # one cell: brute force, exactly
    assert 0 < tests[None] < tests[2] <= 8 * tests[1]


def test_big_sphere_default_grid_tests_far_fewer_faces(cuda):
    v, f, vn, fn = get('sphere136', cuda)
    assert len(vn) > 65536 and len(fn) > 130000
    rng = np.random.default_rng(2)
    pts = (vn[rng.choice(len(vn), 256, replace=False)] * rng.uniform(0.9, 1.1, (256, 1))).astype(F32)
    got = ops.mesh_closest_point(torch.from_numpy(pts).to(cuda), v, f, return_stats=True)
    same(got, reference(('sphere136', 'near'), pts, vn, fn))
    tests = int(got[3].cpu()[0])
    print(f'sphere136: {tests / 256:.1f} point-face tests per query of {len(fn)} faces')
    assert 0 < tests < 256 * len(fn)


def overlap_mesh(cuda):
    """sphere24 plus: one triangle spanning the whole box, a face entered twice more, degenerate faces, an unreferenced vertex"""
    if 'overlap' not in _meshes:
        _, _, vn, fn = get('sphere24', cuda)
        V = len(vn)
        extra_v = np.asarray([[-1, -1, -1], [1, 1, -1], [0, 0, 1], [0.3, 0.3, 0.3]], F32)       # the last: no face uses it
        extra_f = np.asarray([[V, V + 1, V + 2], fn[7], fn[7], [fn[9, 0], fn[9, 1], fn[9, 0]], [fn[11, 2]] * 3, [V, V, V + 1]], I32)
        vv, ff = np.concatenate([vn, extra_v]), np.concatenate([fn[:40], extra_f, fn[40:]]).astype(I32)
        _meshes['overlap'] = (torch.from_numpy(vv).to(cuda), torch.from_numpy(ff).to(cuda), vv, ff)
    return _meshes['overlap']


def test_overlap_lists_with_a_box_spanning_face(cuda):
    v, f, vn, fn = overlap_mesh(cuda)
    grid = ops.mesh_face_grid(v, f)
    K = int(np.prod(grid.cells))
    off, items = grid.cell_offsets.cpu().numpy(), grid.cell_faces.cpu().numpy()
    assert off.shape == (K + 1,) and off[0] == 0 and off[-1] == grid.n_pairs == len(items) and np.all(np.diff(off) >= 1)
    assert grid.n_pairs >= len(fn) + K - 1 and grid.n_pairs > 2 * len(fn)                # pairs >> faces
    spanning = 40
    for l in range(K):
        cell = items[off[l]:off[l + 1]]
        assert np.all(np.diff(cell) > 0) and spanning in cell, l                          # ascending, and the big face everywhere
    # the lists are the restatement's: the cells the fp32 box of every face overlaps
    box, cells = grid.box, grid.cells
    g = lambda x, a: np.clip(np.floor(((x - box[a]).astype(F32) * box[3 + a]).astype(F32)), 0, cells[a] - 1).astype(np.int64)
    tri = vn[fn]                                                                         # [F, 3 vertices, 3 axes]
    lo, hi = [g(tri[:, :, a].min(1), a) for a in range(3)], [g(tri[:, :, a].max(1), a) for a in range(3)]
    count = np.prod([hi[a] - lo[a] + 1 for a in range(3)], axis=0)
    assert count.sum() == grid.n_pairs
    np.testing.assert_array_equal(np.bincount(items, minlength=len(fn)), count)
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.uniform(-1, 1, (700, 3)), vn[fn[42]], vn[fn[7]].mean(0, keepdims=True)]).astype(F32)
    ref = reference(('overlap', 'uniform'), pts, vn, fn)
    assert 40 in ref[0] and 41 not in ref[0] and 42 not in ref[0]                          # the repeated face never beats its first copy
    same(ops.mesh_closest_point(torch.from_numpy(pts).to(cuda), v, f, grid=grid), ref)


def test_one_face_and_non_finite_queries(cuda):
    v = torch.from_numpy(D.cube_mesh(1.0)[0][:3].copy()).to(cuda)
    f = torch.tensor([[0, 1, 2]], device=cuda, dtype=torch.int32)
    rng = np.random.default_rng(9)
    pts = rng.uniform(-2, 2, (130, 3)).astype(F32)
    bad = {3: (np.nan, 0, 0), 64: (0, np.inf, 0), 65: (0, 0, -np.inf), 129: (np.nan, np.nan, np.nan)}
    for i, p in bad.items():
        pts[i] = p
    got = ops.mesh_closest_point(torch.from_numpy(pts).to(cuda), v, f)
    ref = D.closest_point(pts, v.cpu().numpy(), f.cpu().numpy())
    same(got, ref)
    face, point, dist = (t.cpu().numpy() for t in got)
    ok = np.ones(130, bool)
    ok[list(bad)] = False
    assert np.all(face[~ok] == -1) and np.all(np.isnan(dist[~ok])) and np.all(np.isnan(point[~ok]))
    assert np.all(face[ok] == 0) and np.all(np.isfinite(dist[ok])) and np.all(np.isfinite(point[ok]))     # the neighbours in the wave
    # and on a real grid
    v, f, vn, fn = get('sphere24', cuda)
    pts, pn = cluster_samples('sphere24', cuda)
    ref = reference(('sphere24', 'cluster'), pn, vn, fn)
    q = pn[:200].copy()
    q[[0, 63, 64, 150]] = [[np.inf, 0, 0], [0, np.nan, 0], [0, 0, np.inf], [-np.inf, np.inf, 0]]
    face, point, dist = (t.cpu().numpy() for t in ops.mesh_closest_point(torch.from_numpy(q).to(cuda), v, f))
    keep = np.setdiff1d(np.arange(200), [0, 63, 64, 150])
    np.testing.assert_array_equal(face[keep], ref[0][:200][keep])
    np.testing.assert_array_equal(dist[keep], ref[2][:200][keep])
    assert np.all(face[[0, 63, 64, 150]] == -1) and np.all(np.isnan(dist[[0, 63, 64, 150]]))


@pytest.mark.parametrize('k', [1, 2, 3])
def test_samples_equal_restatement(k, cuda):
    v, f, vn, fn = overlap_mesh(cuda)                                                    # with degenerate faces
    pts, fos, w = ops.mesh_sample_faces(v, f, k)
    rp, rf, rw = D.sample_faces(vn, fn, k)
    assert pts.dtype == torch.float32 and fos.dtype == torch.int32 and w.dtype == torch.float64
    np.testing.assert_array_equal(pts.cpu().numpy(), rp)
    np.testing.assert_array_equal(fos.cpu().numpy(), rf)
    np.testing.assert_array_equal(w.cpu().numpy(), rw)
    assert (rw == 0).sum() == 3 * k * k
    e = torch.empty((0, 3), device=cuda, dtype=torch.int32)
    assert [tuple(t.shape) for t in ops.mesh_sample_faces(v, e, k)] == [(0, 3), (0,), (0,)]


def _gpu_report_inputs(a, b, samples, cuda):
    """the restatement's report from the distances the GPU returns (their parity with brute force is tested above)"""
    out = []
    for (v0, f0), (v1, f1) in ((a, b), (b, a)):
        pts, fos, w = ops.mesh_sample_faces(v0, f0, samples)
        face, _, dist = ops.mesh_closest_point(pts, v1, f1)
        out.append((dist.cpu().numpy(), w.cpu().numpy(), D.unit_normals(v0.cpu().numpy(), f0.cpu().numpy()), fos.cpu().numpy(),
                    D.unit_normals(v1.cpu().numpy(), f1.cpu().numpy()), face.cpu().numpy()))
    return out


def test_metrics_parallel_squares(cuda):
    (va, fa), (vb, fb) = D.square_mesh(4, 0.0), D.square_mesh(2, 0.125, flip=True)
    a, b = ((torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda)) for v, f in ((va, fa), (vb, fb)))
    rep = evaluate.mesh_distance_metrics(a, b, samples=3, thresholds=(0.2, 0.1))
    assert rep == D.mesh_distance_metrics(va, fa, vb, fb, samples=3, thresholds=(0.2, 0.1))     # the whole report by brute force
    assert rep['chamfer'] == rep['hausdorff'] == 0.125 and rep['normal_consistency'] == 1.0 and rep['fscore'] == [1.0, 0.0]
    for d in (rep['a_to_b'], rep['b_to_a']):
        assert d['mean'] == d['rms'] == d['max'] == 0.125
    assert evaluate.mesh_distance_metrics(mesh.Mesh(a[0], a[1], None, None), b, samples=3, thresholds=(0.2, 0.1)) == rep


def test_metrics_sphere_against_its_clustered_self(cuda):
    v, f, _, _ = get('sphere24', cuda)
    h = R.step(24)
    cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, 3 * h)
    taus = (0.25 * h, h, 3 * h)
    rep = evaluate.mesh_distance_metrics((v, f), (cv, cf), samples=2, thresholds=taus)
    ins = _gpu_report_inputs((v, f), (cv, cf), 2, cuda)
    want = D.distance_report(D.direction_report(*ins[0], taus), D.direction_report(*ins[1], taus), taus)
    assert rep == want
    assert rep == evaluate.mesh_distance_metrics((v, f), (cv, cf), samples=2, thresholds=taus)       # two runs: the same bits
    print(json.dumps(rep))
    assert 0 < rep['chamfer'] < rep['hausdorff'] < np.sqrt(3.0) * 3 * h                    # no vertex moves further than that
    assert 0 < rep['fscore'][0] < rep['fscore'][1] <= rep['fscore'][2] == 1.0 and 0.9 < rep['normal_consistency'] <= 1
    assert abs(rep['a_to_b']['area'] / (4 * np.pi * 0.36) - 1) < 0.02                   # the sphere of radius 0.6


def test_ops_reject_bad_arguments(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    pts = v[:10].contiguous()
    grid = ops.mesh_face_grid(v, f)
    for bad in (dict(points=pts.double()), dict(points=pts.cpu()), dict(points=pts[:, :2].contiguous()), dict(points=pts.t()[:, :3]),
                dict(points=vn[:10]), dict(verts=v.cpu()), dict(verts=v.half()), dict(faces=f.long()), dict(faces=f[:, :2].contiguous()),
                dict(faces=f[:0].contiguous()), dict(grid='grid'), dict(grid=ops.mesh_face_grid(v.clone(), f))):
        args = dict(points=pts, verts=v, faces=f)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_closest_point(**args)
    ops.mesh_closest_point(pts, v, f, grid=grid)
    f_bad = f.clone()
    f_bad[5, 1] = len(vn)
    v_nan, v_inf = v.clone(), v.clone()
    v_nan[int(fn[3, 0]), 2] = float('nan')
    v_inf[int(fn[8, 1]), 0] = float('inf')
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_face_grid(v, f_bad)
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_closest_point(pts, v, f_bad)
    f_neg = f.clone()
    f_neg[0, 0] = -1
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_sample_faces(v, f_neg, 2)
    for vv in (v_nan, v_inf):
        with pytest.raises(ValueError, match='NaN or infinite'):
            ops.mesh_face_grid(vv, f)
        with pytest.raises(ValueError, match='NaN or infinite'):
            evaluate.mesh_distance_metrics((vv, f), (v, f))
    with pytest.raises(ValueError, match='faces'):
        ops.mesh_face_grid(v, f[:0].contiguous())
    for cells in (0, 513, (2, 2)):
        with pytest.raises(ValueError, match='cells'):
            ops.mesh_face_grid(v, f, cells=cells)
    for k in (0, -1, 1.5, 1025, True):
        with pytest.raises(ValueError, match='k must'):
            ops.mesh_sample_faces(v, f, k)
    with pytest.raises(ValueError, match='samples exceed'):
        ops.mesh_sample_faces(v, f, 1024)
    with pytest.raises(ValueError):
        evaluate.mesh_distance_metrics((v, f), (v, f), samples=0)
    with pytest.raises(ValueError, match='thresholds'):
        evaluate.mesh_distance_metrics((v, f), (v, f), thresholds=(-1.0,))


def test_pair_total_above_int32_is_an_error_not_an_overflow(cuda):
    """cells at the maximum and box-spanning faces: 17 faces x 512^3 cells > 2^31 - 1 pairs."""
    v = torch.tensor([[-1, -1, -1], [1, 1, -1], [0, 0, 1]], device=cuda, dtype=torch.float32)
    f = torch.tensor([[0, 1, 2]] * 17, device=cuda, dtype=torch.int32)
    with pytest.raises(ValueError, match='pairs'):
        ops.mesh_face_grid(v, f, cells=512)
    lib = _lib.load()
    box, cells = (ctypes.c_float * 6)(-1, -1, -1, 256, 256, 256), (ctypes.c_int * 3)(512, 512, 512)
    off = torch.empty(17, device=cuda, dtype=torch.int64)
    meta = torch.zeros(2, device=cuda, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mvip_mesh_distance_grid_count(p(v), p(f), 3, 17, box, cells, p(off), p(meta), ctypes.c_void_p(meta.data_ptr() + 8),
                                             _lib.stream()) == 0
    total, flag = (int(x) for x in meta.cpu())
    assert total == 17 * 512 ** 3 > 2 ** 31 - 1 and flag == 0
    assert off.cpu().tolist() == [i * 512 ** 3 for i in range(17)]                       # a 64-bit scan: nothing wrapped
    assert lib.mvip_mesh_distance_grid_scratch_words(total, cells) == -1
    assert lib.mvip_mesh_distance_grid_fill(p(v), p(f), 3, 17, box, cells, p(off), total, p(off), p(off), p(off), _lib.stream()) == -1
    grid = ops.mesh_face_grid(v, f[:3].contiguous(), cells=(512, 4, 1))                  # the maximum itself is accepted
    assert grid.cells == (512, 4, 1) and grid.n_pairs == 3 * 512 * 4


def test_the_abi_flags_bad_meshes_and_rejects_bad_calls(cuda):
    lib = _lib.load()
    st = _lib.stream()
    v, f, vn, fn = get('sphere24', cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    box, cells = (ctypes.c_float * 6)(-1, -1, -1, 2, 2, 2), (ctypes.c_int * 3)(4, 4, 4)
    off = torch.empty(len(fn), device=cuda, dtype=torch.int64)
    meta = torch.zeros(2, device=cuda, dtype=torch.int64)
    flag = ctypes.c_void_p(meta.data_ptr() + 8)
    f_bad = f.clone()
    f_bad[5, 1] = len(vn)
    v_nan = v.clone()
    v_nan[int(fn[3, 0]), 2] = float('nan')
    for vv, ff, want in ((v, f, 0), (v, f_bad, 1), (v_nan, f, 2), (v_nan, f_bad, 3)):
        assert lib.mvip_mesh_distance_grid_count(p(vv), p(ff), len(vn), len(fn), box, cells, p(off), p(meta), flag, st) == 0
        assert int(meta.cpu()[1]) == want
    one, null = p(off), None
    V, F = len(vn), len(fn)
    assert lib.mvip_mesh_distance_grid_count(p(v), p(f), V, 0, box, cells, p(off), p(meta), flag, st) == -1       # F = 0
    assert lib.mvip_mesh_distance_grid_count(p(v), null, V, F, box, cells, p(off), p(meta), flag, st) == -1
    assert lib.mvip_mesh_distance_query(one, 4, p(v), p(f), V, 0, box, cells, one, one, 8, one, one, one, null, st) == -1
    assert lib.mvip_mesh_distance_query(null, 4, p(v), p(f), V, F, box, cells, one, one, 8, one, one, one, null, st) == -1
    assert lib.mvip_mesh_distance_query(one, -4, p(v), p(f), V, F, box, cells, one, one, 8, one, one, one, null, st) == -1
    assert lib.mvip_mesh_distance_query(null, 0, p(v), p(f), V, F, box, cells, one, one, 8, null, null, null, null, st) == 0    # N = 0
    assert lib.mvip_mesh_sample_faces(p(v), p(f), V, F, 0, one, one, one, flag, st) == -1                          # k < 1
    assert lib.mvip_mesh_sample_faces(p(v), p(f), V, F, 2, one, one, one, null, st) == -1
    torch.cuda.synchronize()


def test_extract_mesh_tool_reports_the_error(cuda, tmp_path, capsys):
    """tools/extract_mesh.py on a tiny synthetic model (seeded weights, 24^3 lattice): with --simplify 3 --report-error it prints the
    report of the finished mesh against the mesh as first extracted; without the flag the file is, byte for byte, what
    extract_mesh + save_ply write (what the tool wrote before the flag existed) and nothing about a report is printed."""
    from oracle.weights import seeded_state_dict
    from tools import extract_mesh as T
    ckpt = str(tmp_path / 'tiny.tar')
    torch.save({'global_step': 0,
                'network_fn_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(2).items()},
                'network_fine_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(1).items()}}, ckpt)
    kw, _ = T.load_model(ckpt, 'mlp', cuda)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 24
    thr = float(mesh.density_grid(kw, lo, hi, res).median())
    plain, direct, simple, reported = (str(tmp_path / n) for n in ('plain.ply', 'direct.ply', 'simple.ply', 'reported.ply'))
    common = [ckpt, '--resolution', str(res), '--threshold', repr(thr)]
    assert T.main(common + ['--out', plain]) == 0
    m = mesh.extract_mesh(kw, lo, hi, resolution=res, threshold=thr)
    mesh.save_ply(direct, m)
    assert open(plain, 'rb').read() == open(direct, 'rb').read()
    assert T.main(common + ['--out', simple, '--simplify', '3']) == 0
    assert 'error report' not in capsys.readouterr().out
    assert T.main(common + ['--out', reported, '--simplify', '3', '--report-error']) == 0
    assert open(simple, 'rb').read() == open(reported, 'rb').read()                    # the flag changes no file
    lines = [ln for ln in capsys.readouterr().out.split('\n') if ln.startswith('error report: ')]
    assert len(lines) == 1
    rep = json.loads(lines[0][len('error report: '):])
    h = 2.0 / (res - 1)
    assert 0 < rep['chamfer'] < rep['hausdorff'] < np.sqrt(3.0) * 3.01 * h and abs(rep['lattice_step'] / h - 1) < 1e-6
    loaded = mesh.load_ply(reported, device=cuda)
    want = evaluate.mesh_distance_metrics(loaded, m, samples=2, thresholds=rep['thresholds'])
    assert rep['hausdorff'] == want['hausdorff'] and rep['chamfer'] == want['chamfer']
