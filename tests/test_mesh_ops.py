"""Mesh clean-up on the GPU (csrc/mesh_ops.hip) against its restatement tests/mesh_ops_numpy.py: corner table, vertex normals,
Taubin smoothing and vertex clustering on meshes that mesh.marching_cubes makes from analytic lattices; bit-reproducibility;
the argument checks of ops and of the C ABI; mesh.smooth / simplify / vertex_normals; tools/extract_mesh.py --smooth --simplify.

Integers (corner table, cluster_of_vertex, faces, colours) must be equal; 'mean' positions bit-equal; quadric positions within
one fp32 ulp of the largest coordinate magnitude outside the borderline clusters (at most 1 % of them); normals and smoothing
within 4 d of the fp64 restatement, d = the restatement's own fp64-against-fp32-rounding gap on the same mesh."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import mesh_ops_numpy as R                               # noqa: E402

from mvip_nerf_amd import _lib, mesh, ops                # noqa: E402

pytestmark = pytest.mark.gpu

_meshes = {}


def big_sphere(x, y, z):
    return R.sphere_field(0.9)(x, y, z)


def cut_valid(n):
    """valid lattice of the cut-open sphere: the points with x < 0.2."""
    ax = np.float32(R.LO[0]) + np.arange(n, dtype=np.float32) * np.float32(R.step(n))
    return np.broadcast_to((ax < 0.2)[:, None, None], (n, n, n)).copy()


MESHES = {
    'sphere24': (24, R.CLUSTER_CASES[0][2], False),
    'cut24': (24, R.CLUSTER_CASES[0][2], True),            # a boundary loop: umbrella counts not doubled there
    'offcentre24': (24, R.CLUSTER_CASES[1][2], False),
    'two_spheres24': (24, R.two_spheres_field, False),
    'torus32': (32, R.torus_field, False),
    # V above 65,536 (a 48^3 sphere of this box has only some 6 k vertices; 136^3 at radius 0.9 has about 70 k)
    'sphere136': (136, big_sphere, False),
}
CASE_MESH = {'sphere24_3': 'sphere24', 'sphere24_2box': 'offcentre24', 'two_spheres24_2.5': 'two_spheres24', 'torus32_6': 'torus32'}


def get(name, cuda):
    """(verts, faces) device tensors and their numpy copies, made once."""
    if name not in _meshes:
        npts, fn, cut = MESHES[name]
        grid = torch.from_numpy(R.lattice(npts, fn)).to(cuda)
        valid = torch.from_numpy(cut_valid(npts)).to(cuda) if cut else None
        v, f, _ = mesh.marching_cubes(grid, 1.0, R.LO, R.HI, valid=valid)
        if cut:                                            # and a vertex no face references
            v = torch.cat([v, torch.tensor([[0.9, 0.9, 0.9]], device=cuda)]).contiguous()
        vn, fn_ = v.cpu().numpy(), f.cpu().numpy()
        vn.setflags(write=False)
        fn_.setflags(write=False)
        _meshes[name] = (v, f, vn, fn_)
    return _meshes[name]


def test_meshes_have_the_shapes_the_kernels_can_go_wrong_at(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    assert 3 * len(fn) > 1024 and (3 * len(fn)) % 1024 != 0
    assert R.directed_edge_balance(fn) == 0
    v, f, vn, fn = get('cut24', cuda)
    assert M.edge_incidence(fn)[1].min() == 1              # a boundary
    assert np.bincount(fn.reshape(-1), minlength=len(vn))[-1] == 0
    assert len(get('sphere136', cuda)[2]) > 65536


@pytest.mark.parametrize('name', list(MESHES))
def test_corner_table_equals_restatement(name, cuda):
    v, f, vn, fn = get(name, cuda)
    off, cor = ops.mesh_corner_table(f, len(vn))
    roff, rcor = R.corner_table(fn, len(vn))
    assert off.dtype == torch.int32 and cor.dtype == torch.int32
    np.testing.assert_array_equal(off.cpu().numpy(), roff)
    np.testing.assert_array_equal(cor.cpu().numpy(), rcor)


def test_corner_table_empty_and_bad_indices(cuda):
    e = torch.empty((0, 3), device=cuda, dtype=torch.int32)
    off, cor = ops.mesh_corner_table(e, 7)
    assert off.tolist() == [0] * 8 and cor.shape == (0,)
    off, cor = ops.mesh_corner_table(e, 0)
    assert off.tolist() == [0] and cor.shape == (0,)
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], device=cuda, dtype=torch.int32)
    off, cor = ops.mesh_corner_table(f, 5)
    assert off.tolist() == [0, 1, 3, 5, 6, 6] and cor.tolist() == [0, 1, 4, 2, 3, 5]
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match='outside'):
            ops.mesh_corner_table(torch.tensor(bad, device=cuda, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_corner_table(f, 0)


@pytest.mark.parametrize('name', ['sphere24', 'cut24', 'two_spheres24', 'sphere136'])
def test_vertex_normals_within_four_rounding_gaps(name, cuda):
    v, f, vn, fn = get(name, cuda)
    n = ops.mesh_vertex_normals(v, f)
    assert n.dtype == torch.float32 and n.shape == v.shape
    ref64 = R.vertex_normals(vn, fn, 'fp64')
    d = float(np.abs(ref64 - R.vertex_normals(vn, fn, 'fp32')).max())
    got = float(np.abs(n.cpu().numpy().astype(np.float64) - ref64).max())
    print(f'{name}: normals d = {d:.3e}, GPU - fp64 restatement = {got:.3e}')
    assert 0 < d <= 2.0 ** -24 and got <= 4 * d
    lone = np.bincount(fn.reshape(-1), minlength=len(vn)) == 0
    assert np.all(n.cpu().numpy()[lone] == 0)
    if name == 'sphere24':
        assert np.all(np.einsum('ij,ij->i', n.cpu().numpy(), vn) > 0)          # outward, as -grad sigma is


@pytest.mark.parametrize('name,iters', [('sphere24', 10), ('cut24', 3), ('two_spheres24', 3), ('sphere136', 2)])
def test_smoothing_within_four_rounding_gaps(name, iters, cuda):
    v, f, vn, fn = get(name, cuda)
    out = ops.mesh_smooth(v, f, iters)
    assert out.dtype == torch.float32 and out.shape == v.shape and out.data_ptr() != v.data_ptr()
    ref64 = R.smooth(vn, fn, iters, rounding='fp64')
    d = float(np.abs(ref64 - R.smooth(vn, fn, iters, rounding='fp32')).max())
    got = float(np.abs(out.cpu().numpy().astype(np.float64) - ref64).max())
    print(f'{name}, {iters} iterations: smoothing d = {d:.3e}, GPU - fp64 restatement = {got:.3e}')
    assert 0 < d <= 2 * iters * 2.0 ** -24 and got <= 4 * d
    lone = np.bincount(fn.reshape(-1), minlength=len(vn)) == 0
    assert np.array_equal(out.cpu().numpy()[lone], vn[lone])                   # vertices without faces do not move
    assert np.array_equal(v.cpu().numpy(), vn)                                 # the input is left alone


def test_smoothing_other_weights_zero_iterations_and_refusals(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    out = ops.mesh_smooth(v, f, 2, lam=0.33, mu=-0.34)
    ref64 = R.smooth(vn, fn, 2, 0.33, -0.34, rounding='fp64')
    d = float(np.abs(ref64 - R.smooth(vn, fn, 2, 0.33, -0.34)).max())
    assert np.abs(out.cpu().numpy() - ref64).max() <= 4 * d
    copy = ops.mesh_smooth(v, f, 0)
    assert torch.equal(copy, v) and copy.data_ptr() != v.data_ptr()
    for kw in (dict(iters=-1), dict(lam=float('nan')), dict(mu=float('inf')), dict(lam=0.0), dict(lam=-0.5), dict(mu=0.0),
               dict(mu=0.1), dict(lam=0.5, mu=-0.4)):
        with pytest.raises(ValueError):
            ops.mesh_smooth(v, f, **kw)
    assert ops.mesh_smooth(v, f, 1, lam=0.5, mu=-0.5).shape == v.shape         # mu = -lam is the boundary, allowed


def run_cluster(cuda, case, placement, dedupe=False, colors=False, repeats=False):
    name, npts, _, steps, origin = next(c for c in R.CLUSTER_CASES if c[0] == case)
    v, f, vn, fn = get(CASE_MESH[case], cuda)
    if repeats:
        fn = np.concatenate([fn, np.roll(fn[::7], 1, axis=1), fn[::11][:, ::-1]]).astype(np.int32)
        f = torch.from_numpy(fn).to(cuda)
    col = np.random.RandomState(3).randint(0, 256, vn.shape).astype(np.uint8) if colors else None
    o = None if origin is None else R.LO
    cell = steps * R.step(npts)
    got = ops.mesh_cluster(v, f, None if col is None else torch.from_numpy(col).to(cuda), o, cell, placement, dedupe)
    return got, R.cluster(vn, fn, col, o, cell, placement, dedupe), vn


def check_integers(got, ref):
    gv, gf, gc, cov = got
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and cov.dtype == torch.int32
    np.testing.assert_array_equal(cov.cpu().numpy(), ref['cluster_of_vertex'])
    np.testing.assert_array_equal(gf.cpu().numpy(), ref['faces'])
    assert gv.shape == ref['verts'].shape
    if ref['colors'] is None:
        assert gc is None
    else:
        assert gc.dtype == torch.uint8
        np.testing.assert_array_equal(gc.cpu().numpy(), ref['colors'])


@pytest.mark.parametrize('case', [c[0] for c in R.CLUSTER_CASES])
def test_cluster_mean_is_bit_equal(case, cuda):
    got, ref, _ = run_cluster(cuda, case, 'mean', colors=True)
    check_integers(got, ref)
    assert np.array_equal(got[0].cpu().numpy().view(np.int32), ref['verts'].view(np.int32))
    assert R.directed_edge_balance(got[1].cpu().numpy()) == 0                  # closed inputs stay closed


@pytest.mark.parametrize('case', [c[0] for c in R.CLUSTER_CASES])
def test_cluster_quadric(case, cuda):
    got, ref, vn = run_cluster(cuda, case, 'quadric')
    check_integers(got, ref)
    inside = R.cell_of(got[0].cpu().numpy(), ref['origin'], ref['inv'], ref['cells'])
    np.testing.assert_array_equal(inside, ref['cell_of_cluster'])              # no representative leaves its cell
    if case not in R.QUADRIC_CASES:
        return
    skip = R.borderline(ref)
    assert skip.mean() <= R.MAX_SKIPPED_SHARE
    ulp = float(np.spacing(np.float32(np.abs(vn).max())))
    diff = np.abs(got[0].cpu().numpy().astype(np.float64) - ref['verts'].astype(np.float64))[~skip]
    print(f'{case}: {skip.sum()} of {len(skip)} clusters borderline, largest difference {diff.max():.3e} (ulp {ulp:.3e})')
    assert diff.max() <= ulp
    assert ref['used_quadric'].mean() > 0.5


def test_cluster_dedupe_and_repeated_faces(cuda):
    got, ref, _ = run_cluster(cuda, 'sphere24_3', 'quadric', dedupe=True, repeats=True)
    check_integers(got, ref)
    plain, pref, _ = run_cluster(cuda, 'sphere24_3', 'quadric', dedupe=False, repeats=True)
    check_integers(plain, pref)
    assert 0 < got[1].shape[0] < plain[1].shape[0]
    cyc = R.canonical_cycles(got[1].cpu().numpy())
    assert len(np.unique(cyc, axis=0)) == len(cyc)


def test_cluster_past_65536_vertices(cuda):
    v, f, vn, fn = get('sphere136', cuda)
    cell = 4.0 * R.step(136)
    got = ops.mesh_cluster(v, f, None, None, cell, 'mean')
    ref = R.cluster(vn, fn, None, None, cell, 'mean')
    check_integers(got, ref)
    assert np.array_equal(got[0].cpu().numpy().view(np.int32), ref['verts'].view(np.int32))
    assert got[1].shape[0] < len(fn) / 10
    gotq = ops.mesh_cluster(v, f, None, None, cell, 'quadric')
    refq = R.cluster(vn, fn, None, None, cell, 'quadric')
    check_integers(gotq, refq)
    skip = R.borderline(refq)
    diff = np.abs(gotq[0].cpu().numpy().astype(np.float64) - refq['verts'].astype(np.float64))[~skip]
    assert diff.max() <= float(np.spacing(np.float32(np.abs(vn).max())))


def test_cluster_edge_cases_and_refusals(cuda):
    v, f, vn, fn = get('cut24', cuda)                                          # a boundary and an unreferenced vertex
    cell = 3.0 * R.step(24)
    got = ops.mesh_cluster(v, f, None, None, cell)
    ref = R.cluster(vn, fn, None, None, cell)
    check_integers(got, ref)
    assert got[3][-1].item() == -1                                             # its cluster has no face: dropped
    e = torch.empty((0, 3), device=cuda, dtype=torch.int32)
    gv, gf, gc, cov = ops.mesh_cluster(v, e, None, None, cell)                 # F = 0
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gc is None and torch.all(cov == -1) and cov.shape == (len(vn),)
    gv, gf, gc, cov = ops.mesh_cluster(torch.empty((0, 3), device=cuda), e, torch.empty((0, 3), device=cuda, dtype=torch.uint8),
                                       None, cell)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gc.shape == (0, 3) and cov.shape == (0,)
    with pytest.raises(ValueError, match='smallest admissible cell'):
        ops.mesh_cluster(v, f, None, None, 1e-4)
    with pytest.raises(ValueError, match='outside the box'):
        ops.mesh_cluster(v, f, None, (0.0, -1.0, -1.0), cell)
    bad = v.clone()
    bad[5, 1] = float('nan')
    with pytest.raises(ValueError, match='NaN or infinite'):
        ops.mesh_cluster(bad, f, None, None, cell)
    with pytest.raises(ValueError, match='NaN or infinite'):
        ops.mesh_cluster(bad, f, None, R.LO, cell)
    with pytest.raises(ValueError, match='placement'):
        ops.mesh_cluster(v, f, None, None, cell, placement='median')
    for c in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='cell'):
            ops.mesh_cluster(v, f, None, None, c)
    fbad = f.clone()
    fbad[3, 2] = len(vn)
    with pytest.raises(ValueError, match='face index'):
        ops.mesh_cluster(v, fbad, None, None, cell)
    with pytest.raises(ValueError, match='face index'):
        ops.mesh_vertex_normals(v, fbad)
    with pytest.raises(ValueError, match='face index'):
        ops.mesh_smooth(v, fbad, 1)


def test_operand_checks(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    calls = (lambda a, b: ops.mesh_vertex_normals(a, b), lambda a, b: ops.mesh_smooth(a, b, 1),
             lambda a, b: ops.mesh_cluster(a, b, None, None, 0.3))
    for call in calls:
        with pytest.raises(ValueError, match='no CPU path'):
            call(v.cpu(), f.cpu())
        with pytest.raises(ValueError, match='must be torch.float32'):
            call(v.double(), f)
        with pytest.raises(ValueError, match='must be torch.int32'):
            call(v, f.long())
        with pytest.raises(ValueError, match=r'\[V, 3\]'):
            call(v.reshape(-1), f)
        with pytest.raises(ValueError, match=r'\[F, 3\]'):
            call(v, f[:, :2].contiguous())
        with pytest.raises(ValueError, match='contiguous'):
            call(v, f.t().contiguous().t())
        with pytest.raises(ValueError, match='tensor on the GPU'):
            call(vn, f)
    with pytest.raises(ValueError, match='no CPU path'):
        ops.mesh_corner_table(f.cpu(), len(vn))
    with pytest.raises(ValueError, match='must be torch.int32'):
        ops.mesh_corner_table(f.long(), len(vn))
    with pytest.raises(ValueError, match='contiguous'):
        ops.mesh_corner_table(f.t().contiguous().t(), len(vn))
    with pytest.raises(ValueError, match='must be torch.uint8'):
        ops.mesh_cluster(v, f, torch.zeros_like(v), None, 0.3)
    with pytest.raises(ValueError, match='colors'):
        ops.mesh_cluster(v, f, torch.zeros((3, 3), device=cuda, dtype=torch.uint8), None, 0.3)


def test_abi_refuses_before_any_device_call(cuda):
    lib = _lib.load()
    buf = torch.zeros(128, device=cuda, dtype=torch.int32)
    null, one, two = ctypes.c_void_p(0), ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 256)
    st = _lib.stream()
    big = 2 ** 31
    box, cells = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1), (ctypes.c_int * 3)(2, 2, 2)
    badcells = (ctypes.c_int * 3)(2, 513, 2)
    assert lib.mvip_mesh_list_scratch_words(-1, 1) == -1 and lib.mvip_mesh_list_scratch_words(big, 1) == -1
    assert lib.mvip_mesh_list_scratch_words(6, 4) == 12 and lib.mvip_mesh_rank_groups(-1) == -1 and lib.mvip_mesh_rank_groups(1025) == 2
    for args in ((null, 3, 1, one, one, one, one), (one, -3, 1, one, one, one, one), (one, 3, -1, one, one, one, one),
                 (one, big, 1, one, one, one, one), (one, 3, big, one, one, one, one), (one, 3, 1, null, one, one, one),
                 (one, 3, 1, one, one, one, null)):
        assert lib.mvip_mesh_corner_table(*args, st) == -1
    for args in ((null, one, 3, 1, one, one, one), (one, one, -1, 1, one, one, one), (one, one, 3, -1, one, one, one),
                 (one, one, big, 1, one, one, one), (one, one, 3, big // 3 + 1, one, one, one), (one, one, 3, 1, one, one, null)):
        assert lib.mvip_mesh_vertex_normals(*args, st) == -1
    for args in ((null, one, 3, 1, one, one, 0.5, two), (one, one, 3, 1, one, one, float('nan'), two), (one, one, 3, 1, one, one, 0.5, null),
                 (one, one, -3, 1, one, one, 0.5, two), (one, one, 3, 1, one, one, 0.5, one)):            # the last: out == verts
        assert lib.mvip_mesh_smooth_pass(*args, st) == -1
    for args in ((null, 3, box, cells, one, one, one, one, one, one, one), (one, -1, box, cells, one, one, one, one, one, one, one),
                 (one, 3, None, cells, one, one, one, one, one, one, one), (one, 3, box, badcells, one, one, one, one, one, one, one),
                 (one, 3, box, cells, null, one, one, one, one, one, one), (one, big, box, cells, one, one, one, one, one, one, one)):
        assert lib.mvip_mesh_cluster_assign(*args, st) == -1
    assert lib.mvip_mesh_gather(null, 3, one, 3, one, st) == -1 and lib.mvip_mesh_gather(one, -1, one, 3, one, st) == -1
    assert lib.mvip_mesh_cluster_place(one, null, one, 3, 1, box, cells, 1.0, 1, one, one, one, one, one, 2, one, null, st) == -1
    assert lib.mvip_mesh_cluster_place(one, null, one, 3, 1, box, cells, -1.0, 1, one, one, one, one, one, 1, one, null, st) == -1
    assert lib.mvip_mesh_cluster_place(null, null, one, 3, 1, box, cells, 1.0, 1, one, one, one, one, one, 1, one, null, st) == -1
    assert lib.mvip_mesh_cluster_faces(null, 1, 1, one, one, 0, one, one, one, one, one, one, one, st) == -1
    assert lib.mvip_mesh_cluster_faces(one, 1, 1, one, one, 2, one, one, one, one, one, one, one, st) == -1
    assert lib.mvip_mesh_cluster_faces(one, -1, 1, one, one, 0, one, one, one, one, one, one, one, st) == -1
    assert lib.mvip_mesh_cluster_emit(one, 1, one, one, one, null, 1, one, one, 3, 2, 1, one, one, null, one, st) == -1    # 2 of 1 faces
    assert lib.mvip_mesh_cluster_emit(one, 1, one, one, one, null, 1, one, one, 3, 1, 1, null, one, null, one, st) == -1
    torch.cuda.synchronize()


def test_every_operation_is_bit_reproducible(cuda):
    v, f, vn, fn = get('torus32', cuda)
    col = torch.from_numpy(np.random.RandomState(5).randint(0, 256, vn.shape).astype(np.uint8)).to(cuda)
    cell = 6.0 * R.step(32)

    def everything(v, f, col):
        off, cor = ops.mesh_corner_table(f, v.shape[0])
        cv, cf, cc, cov = ops.mesh_cluster(v, f, col, None, cell, 'quadric', dedupe=True)
        return (off, cor, ops.mesh_vertex_normals(v, f), ops.mesh_smooth(v, f, 4), cv, cf, cc, cov)

    first, second = everything(v, f, col), everything(v, f, col)
    # the same mesh in other memory, while other work keeps the device busy
    side = torch.cuda.Stream(device=cuda)
    a = torch.randn(2048, 2048, device=cuda)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    third = everything(v.clone(), f.clone(), col.clone())
    side.synchronize()
    for x, y, z in zip(first, second, third):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert x.dtype != torch.float32 or (torch.equal(x.view(torch.int32), y.view(torch.int32)) and
                                            torch.equal(x.view(torch.int32), z.view(torch.int32)))


def test_mesh_wrappers(cuda):
    v, f, vn, fn = get('sphere24', cuda)
    col = torch.from_numpy(np.random.RandomState(7).randint(0, 256, vn.shape).astype(np.uint8)).to(cuda)
    _, _, lattice_normals = mesh.marching_cubes(torch.from_numpy(R.lattice(24, R.CLUSTER_CASES[0][2])).to(cuda), 1.0, R.LO, R.HI)
    m = mesh.Mesh(v, f, lattice_normals, col)
    assert torch.equal(mesh.vertex_normals(m), ops.mesh_vertex_normals(v, f))
    s = mesh.smooth(m, iters=3)
    assert s.faces is m.faces and s.colors is m.colors
    assert torch.equal(s.verts, ops.mesh_smooth(v, f, 3)) and torch.equal(s.normals, ops.mesh_vertex_normals(s.verts, f))
    cell = 3.0 * R.step(24)
    q = mesh.simplify(m, cell)
    cv, cf, cc, _ = ops.mesh_cluster(v, f, col, None, cell, 'quadric', False)
    assert torch.equal(q.verts, cv) and torch.equal(q.faces, cf) and torch.equal(q.colors, cc)
    assert torch.equal(q.normals, ops.mesh_vertex_normals(cv, cf))
    assert M.is_closed(q.faces.cpu().numpy()) or R.directed_edge_balance(q.faces.cpu().numpy()) == 0
    assert mesh.simplify(mesh.Mesh(v, f, lattice_normals, None), cell, placement='mean', origin=R.LO).colors is None
    # Taubin smoothing of a noisy sphere: smoother, and about the same volume
    noisy = (v + 0.01 * torch.randn(v.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(0))).contiguous()
    t = mesh.smooth(mesh.Mesh(noisy, f, lattice_normals, None))
    rms = lambda p: float(p.norm(dim=1).std())
    assert rms(t.verts) < 0.6 * rms(noisy)
    vol = M.signed_volume(noisy.cpu().numpy(), fn)
    assert abs(M.signed_volume(t.verts.cpu().numpy(), fn) - vol) < 0.02 * vol


def test_extract_mesh_tool_smooths_and_simplifies(cuda, tmp_path):
    """tools/extract_mesh.py on a tiny synthetic model (seeded weights, 24^3 lattice): without the new flags the file is,
    byte for byte, what extract_mesh + save_ply write (what the tool wrote before the flags existed); with --simplify 4
    --smooth 5 it holds mesh.simplify(mesh.smooth(...)) of that mesh."""
    from oracle.weights import seeded_state_dict
    from tools import extract_mesh as T
    ckpt = str(tmp_path / 'tiny.tar')
    torch.save({'global_step': 0,
                'network_fn_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(2).items()},
                'network_fine_state_dict': {k: torch.from_numpy(w) for k, w in seeded_state_dict(1).items()}}, ckpt)
    kw, _ = T.load_model(ckpt, 'mlp', cuda)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 24
    thr = float(mesh.density_grid(kw, lo, hi, res).median())
    assert thr > 0
    plain, cleaned, direct = (str(tmp_path / n) for n in ('plain.ply', 'cleaned.ply', 'direct.ply'))
    common = [ckpt, '--resolution', str(res), '--threshold', repr(thr)]
    assert T.main(common + ['--out', plain]) == 0
    m = mesh.extract_mesh(kw, lo, hi, resolution=res, threshold=thr)
    assert m.faces.shape[0] > 100
    mesh.save_ply(direct, m)
    assert open(plain, 'rb').read() == open(direct, 'rb').read()
    assert T.main(common + ['--out', cleaned, '--simplify', '4', '--smooth', '5']) == 0
    head, vert, faces = M.read_ply(cleaned)
    want = mesh.simplify(mesh.smooth(m, 5), 4 * float(np.float32(2.0) / np.float32(res - 1)))     # the tool's largest lattice step
    assert 0 < want.faces.shape[0] < m.faces.shape[0] / 4
    assert f'element vertex {want.verts.shape[0]}' in head and f'element face {want.faces.shape[0]}' in head
    np.testing.assert_array_equal(faces, want.faces.cpu().numpy())
    np.testing.assert_array_equal(np.stack([vert['x'], vert['y'], vert['z']], -1), want.verts.cpu().numpy())
    np.testing.assert_array_equal(np.stack([vert['nx'], vert['ny'], vert['nz']], -1), want.normals.cpu().numpy())
    np.testing.assert_array_equal(np.stack([vert['red'], vert['green'], vert['blue']], -1), want.colors.cpu().numpy())
    assert faces.max() == len(vert) - 1 and faces.min() == 0
