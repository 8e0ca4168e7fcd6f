"""Signed mesh distance on the GPU (csrc/mesh_sdf.hip) against its restatement tests/mesh_sdf_numpy.py: the vertex pseudonormals
within the bound their atan2 allows, and -- fed the kernel's own pseudonormals -- sdist, face, point and feature BIT-EQUAL on
every grid; the sign against the analytic inside test; the band; the lattice mode; mesh.remesh; the metric margin of
Region.from_mesh / OccupancyGrid.from_mesh; the argument checks of ops and of the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402
import mesh_raycast_numpy as C                           # noqa: E402
import mesh_sdf_numpy as S                               # noqa: E402
import test_mesh_distance as TD                          # noqa: E402
import test_mesh_sdf_cpu as TC                           # noqa: E402

from mvip_nerf_amd import _lib, mesh, occupancy, ops, region      # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32, F64 = np.float32, np.int32, np.float64
SMALL = {'tetrahedron': S.tetrahedron, 'spike': S.spike, 'fan_spike': S.fan_spike, 'cube': lambda: D.cube_mesh(0.5),
         'icosphere2': lambda: C.icosphere(2, 0.8)}
MARCHED = ('sphere24', 'cut24', 'torus32')
_meshes, _cases = {}, {}


def get(name, cuda):
    """(verts, faces) device tensors and their numpy copies, made once"""
    if name in MARCHED:
        return TD.get(name, cuda)
    if name not in _meshes:
        vn, fn = SMALL[name]()
        vn, fn = np.ascontiguousarray(vn, F32), np.ascontiguousarray(fn, I32)
        vn.setflags(write=False)
        fn.setflags(write=False)
        _meshes[name] = (torch.from_numpy(vn.copy()).to(cuda), torch.from_numpy(fn.copy()).to(cuda), vn, fn)
    return _meshes[name]


def kernel_P(name, cuda):
    v, f, _, _ = get(name, cuda)
    return ops.mesh_vertex_pseudonormals(v, f)


def case(name, cuda):
    """(points device, points numpy, the kernel's P, the restatement's answer fed that P), made once and left unchanged"""
    if name not in _cases:
        v, f, vn, fn = get(name, cuda)
        pn = S.query_set(vn, fn, 3001, 7)
        if len(pn) % 256 == 0:
            pn = np.concatenate([pn, [[0.1, 0.2, 0.3]]]).astype(F32)
        P = kernel_P(name, cuda)
        ref = S.signed_distance(pn, vn, fn, P=P.cpu().numpy(), prune=len(fn) > 500)
        for a in (pn,) + ref:
            a.setflags(write=False)
        _cases[name] = (torch.from_numpy(pn.copy()).to(cuda), pn, P, ref)
    return _cases[name]


def same(got, ref, what=''):
    sd, face, point, feat = (t.cpu().numpy() for t in got)
    assert sd.dtype == F32 and face.dtype == I32 and point.dtype == F32 and feat.dtype == I32
    np.testing.assert_array_equal(face, ref[1], err_msg=what + ' face')
    np.testing.assert_array_equal(feat, ref[3], err_msg=what + ' feature')
    np.testing.assert_array_equal(sd, ref[0], err_msg=what + ' sdist')        # NaN == NaN here
    np.testing.assert_array_equal(np.signbit(sd), np.signbit(ref[0]), err_msg=what + ' sign')
    np.testing.assert_array_equal(point, ref[2], err_msg=what + ' point')


@pytest.mark.parametrize('name', list(SMALL) + list(MARCHED))
def test_vertex_pseudonormals_within_the_atan2_bound(name, cuda):
    """n_corners(v) * 64 * 2^-53 absolute per component: an OpenCL-class atan2 is within 6 ulp and libm within 1 ulp of
    theta <= pi < 4, under 28 * 2^-53 per term; a few correctly rounded products and sums come on top; the order is the same."""
    v, f, vn, fn = get(name, cuda)
    P = kernel_P(name, cuda)
    assert P.dtype == torch.float64 and tuple(P.shape) == (len(vn), 3)
    want = S.vertex_pseudonormals(vn, fn)
    nc = S.n_corners(fn, len(vn))
    err = np.abs(P.cpu().numpy() - want)
    print(name, 'largest |P - restatement| / 2^-53:', float(err.max() * 2.0 ** 53), 'corners up to', int(nc.max()))
    assert np.all(err <= (nc * 64.0 * 2.0 ** -53)[:, None])
    if name == 'cut24':
        assert nc[-1] == 0 and np.all(P.cpu().numpy()[-1] == 0)                       # the vertex no face references
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize('name', ['tetrahedron', 'fan_spike', 'cube', 'cut24', 'torus32'])
def test_signed_distance_equals_the_restatement_on_every_grid(name, cuda):
    v, f, vn, fn = get(name, cuda)
    pts, pn, P, ref = case(name, cuda)
    assert len(pn) > 1025 and len(pn) % 256 != 0
    zero = ref[4] == 0
    assert zero.sum() >= len(vn) - 1 and not np.any(np.signbit(ref[0][zero]))          # distance 0: a positive sign
    codes = set(np.unique(ref[3]).tolist())
    assert {-1, 0} <= codes and codes & {1, 2, 3} and codes & {4, 5, 6} and (name != 'tetrahedron' or len(codes) == 8)
    assert (ref[1] == -1).sum() == len(S.BAD_ROWS) and (ref[0] < 0).any() and (ref[0] > 0).any()
    twin = ops.mesh_edge_table(f, len(vn)).twin
    for cells in (1, None, (7, 5, 3)):
        grid = ops.mesh_face_grid(v, f, cells=cells)
        got = ops.mesh_signed_distance(pts, v, f, grid=grid, twin=twin, pseudonormals=P, return_feature=True)
        same(got, ref, f'{name} cells={cells}')
        face, point, dist = ops.mesh_closest_point(pts, v, f, grid=grid)
        assert torch.equal(face, got[1])
        np.testing.assert_array_equal(point.cpu().numpy(), got[2].cpu().numpy())
        np.testing.assert_array_equal(dist.cpu().numpy(), got[0].abs().cpu().numpy())
    got = ops.mesh_signed_distance(pts, v, f, return_feature=True)                      # everything built inside
    same(got, ref, name + ' defaults')
    assert len(ops.mesh_signed_distance(pts, v, f)) == 3
    empty = ops.mesh_signed_distance(pts[:0].contiguous(), v, f, return_feature=True)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 3), (0,)]


@pytest.mark.parametrize('name', list(TC.CONVEX))
def test_sign_equals_the_analytic_inside_test_through_the_kernel(name, cuda):
    vn, fn, pn, _, inside = TC.convex_case(name)
    v, f = torch.from_numpy(vn.copy()).to(cuda), torch.from_numpy(fn.copy()).to(cuda)
    sd = ops.mesh_signed_distance(torch.from_numpy(pn.copy()).to(cuda), v, f)[0].cpu().numpy()
    assert len(sd) == TC.N_POINTS and np.all(np.isfinite(sd)) and np.all(sd != 0)
    assert int(np.sum((sd < 0) != inside)) == 0


@pytest.mark.parametrize('name', ['fan_spike', 'torus32'])
def test_band_keeps_exactly_the_queries_within_it_and_their_values(name, cuda):
    v, f, vn, fn = get(name, cuda)
    pts, pn, P, ref = case(name, cuda)
    free = ops.mesh_signed_distance(pts, v, f, pseudonormals=P, return_feature=True)
    same(free, ref)
    d2 = ref[4]
    span = float(np.ptp(vn, axis=0).max())
    for B in (0.03 * span, 0.25 * span):
        with np.errstate(invalid="ignore"):
            inband = d2 <= float(B) * float(B)                                             # NaN (the bad rows): out
        assert 0 < inband.sum() < len(pn) - len(S.BAD_ROWS)
        for cells in (1, None, (7, 5, 3)):
            grid = ops.mesh_face_grid(v, f, cells=cells)
            got = ops.mesh_signed_distance(pts, v, f, grid=grid, pseudonormals=P, max_dist=B, return_feature=True)
            np.testing.assert_array_equal(got[1].cpu().numpy() >= 0, inband, err_msg=f'B={B} cells={cells}')
            for g, u in zip(got, free):
                g, u = g.cpu().numpy(), u.cpu().numpy()
                np.testing.assert_array_equal(g[inband], u[inband])
            assert np.all(np.isnan(got[0].cpu().numpy()[~inband])) and np.all(np.isnan(got[2].cpu().numpy()[~inband]))
            assert np.all(got[3].cpu().numpy()[~inband] == -1)
        want = S.signed_distance(pn, vn, fn, P=P.cpu().numpy(), max_dist=B, closest=(ref[1], _unrounded(ref, pn, vn, fn), ref[4], ref[3]))
        same(ops.mesh_signed_distance(pts, v, f, pseudonormals=P, max_dist=B, return_feature=True), want, f'B={B}')


def _unrounded(ref, pn, vn, fn):
    """q unrounded of a cached answer: recomputed for the winning faces alone"""
    face = ref[1]
    ok = face >= 0
    v = vn.astype(F64)
    tri = v[fn[np.where(ok, face, 0)]]
    p = pn.astype(F64)
    with np.errstate(invalid='ignore'):                        # (the NaN and inf rows)
        _, q, _ = S._point_triangle(tuple(p[:, t] for t in range(3)), tuple(tri[:, 0, t] for t in range(3)),
                                    tuple(tri[:, 1, t] for t in range(3)), tuple(tri[:, 2, t] for t in range(3)))
    return np.where(ok[:, None], np.stack(q, -1), np.nan)


@pytest.mark.parametrize('res', [(9, 6, 5), 33])
def test_lattice_mode_equals_points_mode_on_the_grid_axes(res, cuda):
    v, f, vn, fn = get('icosphere2', cuda)
    lo, hi = (-1.0, -0.9, -1.1), (1.0, 1.1, 0.9)
    ax = mesh.grid_axes(lo, hi, res, cuda)
    pts = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3).contiguous()
    counts = tuple(len(a) for a in ax)
    np.testing.assert_array_equal(pts.cpu().numpy(), S.lattice_points(*ops.mesh_lattice(lo, hi, res)))
    P = kernel_P('icosphere2', cuda)
    tests = {}
    for B in (None, 0.15):
        sd, face = ops.mesh_signed_distance_lattice(v, f, lo, hi, res, max_dist=B, pseudonormals=P)
        assert tuple(sd.shape) == counts == tuple(face.shape) and sd.dtype == torch.float32 and face.dtype == torch.int32
        want = ops.mesh_signed_distance(pts, v, f, max_dist=B, pseudonormals=P)
        np.testing.assert_array_equal(sd.reshape(-1).cpu().numpy(), want[0].cpu().numpy())
        assert torch.equal(face.reshape(-1), want[1])
        again = ops.mesh_signed_distance_lattice(v, f, lo, hi, res, max_dist=B, pseudonormals=P, return_stats=True)      # the counting variant
        np.testing.assert_array_equal(again[0].cpu().numpy(), sd.cpu().numpy())
        tests[B] = int(again[2].cpu()[0])
        inside = (sd < 0).sum().item()
        assert (B is None and 0 < inside < sd.numel()) or (B is not None and 0 < (face >= 0).sum().item() < sd.numel())
    assert 0 < tests[0.15] < tests[None]                                               # the band ends the walk of a far point early


def test_remesh_gives_a_closed_sphere_at_the_offset(cuda):
    vn, fn = C.icosphere(3, 0.8)
    v, f = torch.from_numpy(np.ascontiguousarray(vn, F32)).to(cuda), torch.from_numpy(np.ascontiguousarray(fn, I32)).to(cuda)
    src = mesh.Mesh(v, f, None, None)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    step = float(max(ops.mesh_lattice(lo, hi, 48)[1]))
    for offset in (0.0, 2 * step, -2 * step):
        out = mesh.remesh(src, resolution=48, offset=offset, band=4 * step, bound_min=lo, bound_max=hi)
        assert out.colors is None and out.faces.shape[0] > 1000
        t = mesh.topology(out)
        assert t['closed'] and t['oriented'] and t['components'] == 1 and t['genus'] == 0, t
        dist = ops.mesh_closest_point(out.verts, v, f)[2].cpu().numpy()
        print('offset', offset, 'distance of the new vertices:', float(dist.min()), '..', float(dist.max()), 'step', step)
        # the distance is 1-Lipschitz, so the level crossing on a lattice edge lies within one step of the level
        assert np.all(np.abs(dist - abs(offset)) <= step)
        sd = ops.mesh_signed_distance(out.verts, v, f)[0].cpu().numpy()
        assert offset == 0.0 or np.all(np.sign(sd) == np.sign(offset))
    out = mesh.remesh(src, resolution=48)                                              # the default box and band
    t = mesh.topology(out)
    assert t['closed'] and t['oriented'] and t['components'] == 1 and t['genus'] == 0
    with pytest.raises(ValueError, match='band'):
        mesh.remesh(src, resolution=48, offset=2.5 * step, band=4 * step, bound_min=lo, bound_max=hi)
    with pytest.raises(ValueError):
        mesh.remesh(src, resolution=48, bound_min=lo)
    sd, valid = mesh.sdf_grid(src, lo, hi, 48)
    assert tuple(sd.shape) == (48, 48, 48) and valid.dtype == torch.bool and 0 < valid.sum().item() < valid.numel()
    assert torch.isnan(sd[~valid]).all() and (sd[valid].abs() <= 3 * step * (1 + 1e-6)).all()
    got = mesh.signed_distance(src, [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])[0].cpu().numpy()
    assert got[0] < -0.7 and got[1] > 1.1


def _pack(bits):
    bits = np.asarray(bits, bool).reshape(-1)
    pad = np.zeros((len(bits) + 31) // 32 * 32, bool)
    pad[:len(bits)] = bits
    return (pad.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32).view(I32)


@pytest.mark.parametrize('margin', [0.1, -0.1])
def test_margin_sets_or_clears_the_cells_whose_centre_is_that_near(margin, cuda):
    v, f, vn, fn = get('cube', cuda)
    src = mesh.Mesh(v, f, None, None)
    bmin, bmax, cells = (-1.0, -1.1, -0.9), (1.1, 1.0, 1.2), (16, 16, 16)
    base = region.Region.from_mesh(src, bmin, bmax, cells, dilate=0).words.cpu().numpy()
    lo, hi = np.asarray(bmin, F32), np.asarray(bmax, F32)
    w = (hi.astype(F64) - lo.astype(F64)) / np.asarray(cells, F64)
    first, last = (lo.astype(F64) + w / 2).astype(F32), (hi.astype(F64) - w / 2).astype(F32)
    h = np.asarray([(last[a] - first[a]) / F32(cells[a] - 1) for a in range(3)], F32)
    centres = S.lattice_points(first, h, cells)
    near = _pack(S.signed_distance(centres, vn, fn, max_dist=abs(margin))[1] >= 0)
    assert 0 < np.unpackbits(near.view(np.uint8)).sum() < 16 ** 3
    want = (base | near) if margin > 0 else (base & ~near)
    assert not np.array_equal(want, base)
    for cls in (region.Region, occupancy.OccupancyGrid):
        got = cls.from_mesh(src, bmin, bmax, cells, dilate=0, margin=margin)
        np.testing.assert_array_equal(got.words.cpu().numpy(), want)
        np.testing.assert_array_equal(cls.from_mesh(src, bmin, bmax, cells, dilate=0, margin=None).words.cpu().numpy(), base)
    one = region.Region.from_mesh(src, bmin, bmax, cells, dilate=1, margin=margin)      # the margin comes before the dilation
    assert torch.equal(one.words, region.Region(one.bmin, one.bmax, cells, torch.from_numpy(want).to(cuda)).dilate(1).words)


def test_margin_none_is_the_voxelisation_alone_and_one_cell_is_refused(cuda):
    v, f, vn, fn = get('cube', cuda)
    src = mesh.Mesh(v, f, None, None)
    bmin, bmax, cells = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (16, 16, 16)
    grid, _ = mesh.voxelize(src, bmin, bmax, cells, mode='both')
    for rounds in (0, 1):
        want = region.Region(grid.bmin, grid.bmax, cells, grid.words).dilate(rounds).words
        assert torch.equal(region.Region.from_mesh(src, bmin, bmax, cells, dilate=rounds).words, want)
        assert torch.equal(region.Region.from_mesh(src, bmin, bmax, cells, dilate=rounds, margin=None).words, want)
        assert torch.equal(occupancy.OccupancyGrid.from_mesh(src, bmin, bmax, cells, dilate=rounds, margin=None).words, want)
    for cls in (region.Region, occupancy.OccupancyGrid):
        with pytest.raises(ValueError, match='two cells'):
            cls.from_mesh(src, bmin, bmax, 1, margin=0.1)
        with pytest.raises(ValueError, match='finite'):
            cls.from_mesh(src, bmin, bmax, cells, margin=float('nan'))
        cls.from_mesh(src, bmin, bmax, 1)                                              # without a margin one cell is fine


def test_ops_reject_bad_arguments(cuda):
    v, f, vn, fn = get('icosphere2', cuda)
    pts = v[:10].contiguous()
    twin, P = ops.mesh_edge_table(f, len(vn)).twin, kernel_P('icosphere2', cuda)
    for bad in (dict(points=pts.double()), dict(points=pts.cpu()), dict(points=pts[:, :2].contiguous()), dict(points=pts.t()[:, :3]),
                dict(points=vn[:10]), dict(verts=v.cpu()), dict(verts=v.half()), dict(faces=f.long()), dict(faces=f[:0].contiguous()),
                dict(grid='grid'), dict(grid=ops.mesh_face_grid(v.clone(), f)), dict(twin=twin[:-1].contiguous()), dict(twin=twin.long()),
                dict(twin=twin.cpu()), dict(pseudonormals=P.float()), dict(pseudonormals=P[:-1].contiguous()), dict(pseudonormals='P'),
                dict(max_dist=-1.0), dict(max_dist=float('nan'))):
        args = dict(points=pts, verts=v, faces=f)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance(**args)
    ops.mesh_signed_distance(pts, v, f, twin=twin, pseudonormals=P, max_dist=0.0)
    f_bad = f.clone()
    f_bad[5, 1] = len(vn)
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_signed_distance(pts, v, f_bad)
    with pytest.raises(ValueError, match='outside'):
        ops.mesh_vertex_pseudonormals(v, f_bad)
    with pytest.raises(ValueError):
        ops.mesh_vertex_pseudonormals(v.cpu(), f)
    assert tuple(ops.mesh_vertex_pseudonormals(v, f[:0].contiguous()).shape) == (len(vn), 3)
    for bad in (dict(resolution=1), dict(resolution=(4, 4)), dict(bound_min=(0, 0)), dict(bound_max=(1, 1, float('inf'))),
                dict(bound_max=(1, 1, -1)), dict(resolution=2048), dict(max_dist=-0.5)):
        args = dict(verts=v, faces=f, bound_min=(-1, -1, -1), bound_max=(1, 1, 1), resolution=4)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance_lattice(**args)


def test_the_abi_rejects_bad_calls(cuda):
    lib = _lib.load()
    st = _lib.stream()
    v, f, vn, fn = get('icosphere2', cuda)
    V, F = len(vn), len(fn)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    box, cells = (ctypes.c_float * 6)(-1, -1, -1, 2, 2, 2), (ctypes.c_int * 3)(4, 4, 4)
    bad_box = (ctypes.c_float * 6)(-1, -1, -1, 2, 0, 2)
    words = torch.zeros(4 * V + 16, device=cuda, dtype=torch.int64)
    one, null = p(words), None
    inf = float('inf')
    lo, h, n3 = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_int * 3)(2, 2, 2)
    h0, n0 = (ctypes.c_float * 3)(0.5, 0, 0.5), (ctypes.c_int * 3)(2, 0, 2)
    pn = lib.mvip_mesh_vertex_pseudonormals
    assert pn(p(v), p(f), -1, F, one, one, one, st) == -1
    assert pn(p(v), p(f), V, -1, one, one, one, st) == -1
    assert pn(null, p(f), V, F, one, one, one, st) == -1
    assert pn(p(v), null, V, F, one, one, one, st) == -1
    assert pn(p(v), p(f), V, F, null, one, one, st) == -1
    assert pn(p(v), p(f), V, F, one, null, one, st) == -1
    assert pn(p(v), p(f), V, F, one, one, null, st) == -1
    assert pn(null, null, 0, 0, null, null, null, st) == 0                               # nothing to do
    sd = lib.mvip_mesh_signed_distance
    ok = dict(points=one, lo=null, h=null, counts=null, N=4, verts=p(v), faces=p(f), V=V, F=F, box=box, cells=cells, offsets=one,
              cell_faces=one, pairs=8, twin=one, P=one, B=inf, sdist=one, face=one, point=one, feature=one, stats=null)
    def run(**kw):
        a = dict(ok)
        a.update(kw)
        return sd(a['points'], a['lo'], a['h'], a['counts'], a['N'], a['verts'], a['faces'], a['V'], a['F'], a['box'], a['cells'],
                  a['offsets'], a['cell_faces'], a['pairs'], a['twin'], a['P'], a['B'], a['sdist'], a['face'], a['point'], a['feature'], a['stats'], st)
    for kw in (dict(F=0), dict(V=0), dict(N=-4), dict(points=null), dict(verts=null), dict(faces=null), dict(box=bad_box), dict(box=null),
               dict(cells=null), dict(offsets=null), dict(cell_faces=null), dict(pairs=-1), dict(twin=null), dict(P=null), dict(B=-1.0),
               dict(B=float('nan')), dict(sdist=null), dict(face=null), dict(lo=lo), dict(lo=lo, h=h, counts=n3, N=8),
               dict(points=null, lo=lo, h=h, counts=n3, N=7), dict(points=null, lo=lo, h=h0, counts=n3, N=8),
               dict(points=null, lo=lo, h=h, counts=n0, N=0), dict(points=null, lo=lo, h=null, counts=n3, N=8)):
        assert run(**kw) == -1, kw
    assert run(points=null, N=0, sdist=null, face=null, point=null, feature=null) == 0           # N = 0
    torch.cuda.synchronize()
