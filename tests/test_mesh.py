"""Mesh export on the GPU: the marching-cubes passes of csrc/mcubes.hip against the numpy restatement (tests/mc_numpy.py)
-- identical faces in the same order, the same vertex count, vertices within 1e-6 of the box extent, normal cosines
>= 0.9999 -- on analytic and random fields; empty surfaces and a non-finite grid; a closed sphere; density_grid against
the models' own query functions; extract_mesh end to end with colours and a PLY file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402

from mvip_nerf_amd import mesh                           # noqa: E402

pytestmark = pytest.mark.gpu


def axes(shape, lo, hi):
    return [lo[a] + np.arange(shape[a], dtype=np.float32) * ((hi[a] - lo[a]) / np.float32(shape[a] - 1))
            for a in range(3)]


def field(shape, lo, hi, fn):
    x, y, z = np.meshgrid(*axes(shape, np.asarray(lo, np.float32), np.asarray(hi, np.float32)), indexing='ij')
    return np.ascontiguousarray(fn(x, y, z), dtype=np.float32)


def sphere(x, y, z, r=0.6):
    return 2.0 - np.sqrt(x * x + y * y + z * z) / r


def blobs(x, y, z):
    rs = np.random.RandomState(11)
    out = np.zeros_like(x)
    for _ in range(6):
        c, s, a = rs.uniform(-0.6, 0.6, 3), rs.uniform(0.12, 0.3), rs.uniform(0.8, 2.0)
        out = out + a * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    return out


def compare(grid, iso, lo, hi, cuda):
    v, f, n = mesh.marching_cubes(torch.from_numpy(grid).to(cuda), iso, lo, hi)
    rv, rf, rn = M.marching_cubes(grid, iso, lo, hi)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    assert v.shape == (len(rv), 3) and n.shape == (len(rv), 3)
    np.testing.assert_array_equal(f.cpu().numpy(), rf)
    extent = float(np.max(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    np.testing.assert_allclose(v.cpu().numpy(), rv, rtol=0, atol=1e-6 * extent)
    hn = n.cpu().numpy()
    ok = np.linalg.norm(rn, axis=1) > 0
    cos = np.einsum('ij,ij->i', hn[ok], rn[ok])
    assert cos.min() >= 0.9999
    assert len(rf) > 0
    return v, f, n


def test_sphere_65_matches_restatement(cuda):
    lo, hi = (-1, -1, -1), (1, 1, 1)
    compare(field((65, 65, 65), lo, hi, sphere), 1.0, lo, hi, cuda)


def test_noncubic_anisotropic_matches_restatement(cuda):
    lo, hi = (-1.5, -0.4, 0.25), (2.0, 0.9, 1.0)
    fn = lambda x, y, z: 1.0 + np.sin(2.0 * x) * np.cos(5.0 * y) + np.sin(9.0 * z) * 0.5
    compare(field((97, 80, 71), lo, hi, fn), 1.2, lo, hi, cuda)


def test_gaussian_blobs_match_restatement(cuda):
    lo, hi = (-1, -1, -1), (1, 1, 1)
    compare(field((96, 96, 96), lo, hi, blobs), 0.5, lo, hi, cuda)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_fields_match_restatement_and_repeat_bitwise(seed, cuda):
    g = np.random.RandomState(seed).choice(np.array([-1.0, 1.0], np.float32), size=(24, 24, 24))
    lo, hi = (0, 0, 0), (1, 1, 1)
    v, f, n = compare(g, 0.5, lo, hi, cuda)
    v2, f2, n2 = mesh.marching_cubes(torch.from_numpy(g).to(cuda), 0.5, lo, hi)
    assert torch.equal(v, v2) and torch.equal(f, f2) and torch.equal(n, n2)


def test_empty_surfaces_and_nonfinite_grid(cuda):
    for g in (torch.zeros(9, 10, 11, device=cuda), torch.full((9, 10, 11), 2.0, device=cuda)):
        v, f, n = mesh.marching_cubes(g, 1.0, (0, 0, 0), (1, 1, 1))
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    g = torch.from_numpy(field((20, 20, 20), (-1, -1, -1), (1, 1, 1), sphere)).to(cuda)
    g[3, 4, 5] = float('nan')
    with pytest.raises(ValueError):
        mesh.marching_cubes(g, 1.0, (-1, -1, -1), (1, 1, 1))
    g[3, 4, 5] = float('inf')
    with pytest.raises(ValueError):
        mesh.marching_cubes(g, 1.0, (-1, -1, -1), (1, 1, 1))


def two_far_spheres(x, y, z):
    d1 = np.sqrt((x - 20.3) ** 2 + (y - 30.7) ** 2 + (z - 7.4) ** 2)
    d2 = np.sqrt((x - 740.3) ** 2 + (y - 700.7) ** 2 + (z - 8.6) ** 2)
    return 2.0 - np.minimum(d1, d2) / 6.0


def test_scan_carry_past_one_chunk_matches_restatement(cuda):
    """9216 workgroups: the scan of the workgroup totals runs a second 8192-record chunk.  One sphere lies in the first
    chunk's points, the other past workgroup 8192, so the second sphere's vertex ids and face slots are right only if both
    carried totals (vertices, triangles) are."""
    shape, lo, hi = (768, 768, 16), (0, 0, 0), (767, 767, 15)
    grid = field(shape, lo, hi, two_far_spheres)
    ins = grid >= 1.0
    crossing = np.zeros(shape, bool)                       # points that own a crossing edge (+x, +y, +z)
    crossing[:-1] |= ins[:-1] != ins[1:]
    crossing[:, :-1] |= ins[:, :-1] != ins[:, 1:]
    crossing[:, :, :-1] |= ins[:, :, :-1] != ins[:, :, 1:]
    n = np.nonzero(crossing.reshape(-1))[0]
    split = 8192 * 1024
    assert grid.size == 9216 * 1024 and (n < split).sum() == 508 and (n >= split).sum() == 508
    v, f, _ = compare(grid, 1.0, lo, hi, cuda)
    assert v.shape == (1384, 3) and f.shape == (2760, 3)
    assert M.is_closed(f.cpu().numpy())


def test_sphere_129_closed(cuda):
    r = 0.6
    lo, hi = (-1, -1, -1), (1, 1, 1)
    v, f, n = mesh.marching_cubes(torch.from_numpy(field((129, 129, 129), lo, hi, sphere)).to(cuda), 1.0, lo, hi)
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    assert M.is_closed(f)
    assert M.euler(v, f) == 2
    vol = M.signed_volume(v, f)
    assert abs(vol - 4 / 3 * np.pi * r ** 3) <= 0.01 * 4 / 3 * np.pi * r ** 3
    assert np.all(np.einsum('ij,ij->i', n, v) > 0)


def _mlp_model(cuda):
    import bench
    from mvip_nerf_amd import run
    from oracle.weights import seeded_state_dict
    _, te, _, _, _ = run.create_nerf(bench.make_args(), device=cuda)
    for net, seed in ((te['network_fn'], 2), (te['network_fine'], 1)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
    return te


def _tcnn_model(cuda):
    import types
    from mvip_nerf_amd import run
    args = types.SimpleNamespace(
        use_viewdirs=True, N_importance=64, alpha_model_path=None, netchunk=65536, lrate=1e-2, basedir='/tmp/x',
        expname='none', ft_path=None, no_reload=True, perturb=0., N_samples=64, white_bkgd=True, raw_noise_std=0.,
        dataset_type='llff', no_ndc=True, lindisp=True)
    torch.manual_seed(0)
    _, te, _, _, _ = run.create_nerf_tcnn(args, cuda)
    with torch.no_grad():                                 # a table with visible structure (the seeded one is ~1e-4)
        g = torch.Generator().manual_seed(5)
        te['network_fine'].encoder.params.copy_((torch.rand(te['network_fine'].encoder.params.shape, generator=g) * 2 - 1))
    return te


@pytest.mark.parametrize('model', ['mlp', 'tcnn'])
def test_density_grid_equals_query(model, cuda):
    te = _mlp_model(cuda) if model == 'mlp' else _tcnn_model(cuda)
    lo, hi, res = (-0.7, -0.5, -0.6), (0.8, 0.6, 0.4), (33, 29, 31)
    g = mesh.density_grid(te, lo, hi, res, chunk=4096)
    assert g.shape == res and g.dtype == torch.float32
    xs, ys, zs = mesh.grid_axes(lo, hi, res, cuda)
    X, Y, Z = torch.meshgrid(xs, ys, zs, indexing='ij')
    pts = torch.stack([X, Y, Z], -1).reshape(-1, 1, 3)
    dirs = torch.zeros(pts.shape[0], 3, device=cuda)
    dirs[:, 2] = 1.0
    with torch.no_grad():
        ref = te['network_query_fn'](pts, dirs, te['network_fine'])[:, 0, 3].reshape(res)
    np.testing.assert_allclose(g.cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=1e-6 * float(ref.abs().max()))
    g2 = mesh.density_grid(te, lo, hi, res, chunk=1000)
    assert torch.equal(g, g2)
    # grid points are where the kernels put the mesh vertices' lattice
    np.testing.assert_array_equal(xs.cpu().numpy(), axes(res, np.float32(lo), np.float32(hi))[0])


def test_extract_mesh_mlp(cuda, tmp_path):
    te = _mlp_model(cuda)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 40
    grid = mesh.density_grid(te, lo, hi, res)
    thr = float(grid.median())
    assert thr > 0
    m = mesh.extract_mesh(te, lo, hi, resolution=res, threshold=thr)
    v, f, n = mesh.marching_cubes(grid, thr, lo, hi)
    assert len(f) > 0
    assert torch.equal(m.verts, v) and torch.equal(m.faces, f) and torch.equal(m.normals, n)
    assert m.colors.dtype == torch.uint8 and m.colors.shape == v.shape
    with torch.no_grad():
        raw = te['network_query_fn'](v[:, None, :], -n, te['network_fine'])[:, 0]
    direct = (torch.sigmoid(raw[:, :3]) * 255.0).cpu().numpy()
    assert np.max(np.abs(m.colors.cpu().numpy().astype(np.float64) - direct)) <= 1.0
    p = str(tmp_path / 'mesh.ply')
    mesh.save_ply(p, m)
    head, vert, faces = M.read_ply(p)
    assert f'element vertex {len(v)}' in head and f'element face {len(f)}' in head
    np.testing.assert_array_equal(faces, f.cpu().numpy())
    np.testing.assert_array_equal(np.stack([vert['x'], vert['y'], vert['z']], -1), v.cpu().numpy())
    np.testing.assert_array_equal(np.stack([vert['red'], vert['green'], vert['blue']], -1), m.colors.cpu().numpy())
