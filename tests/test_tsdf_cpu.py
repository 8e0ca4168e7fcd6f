"""TSDF depth-map fusion and marching cubes on observed cells, without a GPU: the numpy restatement (tests/tsdf_numpy.py) against
itself in two precisions and against analytic scenes, and the argument checks of the two new C-ABI entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M                                     # noqa: E402
import tsdf_numpy as R                                   # noqa: E402

from mvip_nerf_amd import _lib                           # noqa: E402

MAX_EXCLUDED = 0.01
EINVAL = -1
P0 = None            # NULL

CASES = {'trial': R.trial_case, 'plane17': lambda: R.plane_case(R.PLANE_LATTICES[0]), 'plane33': lambda: R.plane_case(R.PLANE_LATTICES[1])}
_YARD = {}


def yard(name):
    if name not in _YARD:
        case = CASES[name]()
        _YARD[name] = (case, R.yardstick(*R.args_of(case)))
    return _YARD[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_exclusions_are_rare_and_the_two_precisions_count_alike(name):
    case, y = yard(name)
    print(f'{name}: excluded {y["excluded_share"]:.4%}, e32 {y["e32"]:.3g}, counts differing off them {y["count32_differs"]}')
    assert y['excluded_share'] <= MAX_EXCLUDED
    assert y['count32_differs'] == 0
    V = case['disp'].shape[0]
    for t, c in ((y['tsdf'], y['count']), (y['tsdf32'], y['count32'])):                  # well formed everywhere, excluded or not
        assert t.shape == c.shape == tuple(case['resolution'])
        assert np.all((t >= -1) & (t <= 1)) and np.all((c >= 0) & (c <= V))
        assert np.all(t[c == 0] == 1)
    assert (y['count'] == V).any() and (y['count'] == 0).any()                           # seen by all, and unobserved points
    assert y['e32'] < 1e-4                                                               # fp32 rounding, not another decision


def test_generic_poses():
    """Every angle non-zero and no camera centre on a lattice plane (else a lattice row sits on a pixel-rounding boundary)."""
    for name in sorted(CASES):
        case, _ = yard(name)
        axes = R.lattice(case['bound_min'], case['bound_max'], case['resolution'], np.float64)
        for p in case['poses'].astype(np.float64):
            assert np.all(np.abs(p[:, :3][~np.eye(3, dtype=bool)]) > 1e-4)               # no rotation about one axis alone
            for a in range(3):
                h = axes[a][1] - axes[a][0]
                r = (p[a, 3] - axes[a][0]) / h
                assert abs(r - round(r)) > 1e-3


def test_masks_and_bad_disparities_unsee_pixels_only():
    case = R.trial_case()
    args = R.args_of(case)
    t0, c0 = R.fuse(*args, dtype=np.float32)
    V, H, W = case['disp'].shape
    m = np.ones((V, H, W), bool)
    m[1] = False
    t1, c1 = R.fuse(*args, masks=m, dtype=np.float32)
    keep = [0, 2]
    t2, c2 = R.fuse(case['disp'][keep], case['poses'][keep], *args[2:], dtype=np.float32)
    assert np.array_equal(c1, c2) and np.array_equal(t1.view(np.int32), t2.view(np.int32))
    py, px = R.hit_pixel(case, 0)
    for bad in (np.nan, np.inf, 0.0, -0.5):
        d = case['disp'].copy()
        d[0, py, px] = bad
        mm = np.ones((V, H, W), bool)
        mm[0, py, px] = False
        tb, cb = R.fuse(d, *args[1:], dtype=np.float32)
        tm, cm = R.fuse(case['disp'], *args[1:], masks=mm, dtype=np.float32)
        assert np.array_equal(cb, cm) and np.array_equal(tb.view(np.int32), tm.view(np.int32))
        assert (cb != c0).any() and (cb <= c0).all()


@pytest.mark.parametrize('name', ['plane17', 'plane33'])
def test_restated_plane_mesh_lies_on_the_plane(name):
    case, y = yard(name)
    g, valid = R.mc_lattice(y['tsdf32'], y['count32'])
    verts, faces, normals = R.marching_cubes_valid(g, valid, 1.0, case['bound_min'], case['bound_max'])
    assert len(faces) > 100 and np.array_equal(np.unique(faces), np.arange(len(verts)))
    dist, cos = R.plane_mesh_figures(verts, normals, case)
    print(f'{name}: {len(verts)} vertices, {len(faces)} triangles, farthest {dist:.3f} of a step, smallest cosine {cos:.4f}')
    assert dist <= 0.5
    assert cos >= 0.9


def test_masking_removes_the_shell_between_observed_and_unobserved_space():
    case, y = yard('trial')
    g, valid = R.mc_lattice(y['tsdf32'], y['count32'])
    live = R.live_cells(valid)
    crossing = M.COUNTS[M.cube_indices(g, 1.0)] > 0
    print(f'trial: {int(crossing.sum())} surface-crossing cells, {int((crossing & live).sum())} of them live')
    assert R.triangles_in_dead_cells(g, valid, 1.0) > 0                                  # the unmasked mesh grows the shell
    uv, uf, _ = M.marching_cubes(g, 1.0, case['bound_min'], case['bound_max'])
    verts, faces, _, cells = R.marching_cubes_valid(g, valid, 1.0, case['bound_min'], case['bound_max'], return_cells=True)
    assert 0 < len(faces) < len(uf)
    assert live.reshape(-1)[_cell_index(cells, g.shape)].all()                          # every triangle sits in a live cell
    assert np.array_equal(np.unique(faces), np.arange(len(verts)))                       # no unreferenced vertex, none missing
    # the masked mesh is the unmasked one's triangles in live cells, vertex for vertex
    want = {tuple(np.round(uv[f].astype(np.float64), 6).reshape(-1)) for f in uf}
    assert all(tuple(np.round(verts[f].astype(np.float64), 6).reshape(-1)) in want for f in faces)


def _cell_index(cells, shape):
    """Index into live_cells(...).reshape(-1) of the cells given by their origin points' linear indices."""
    i, j, k = np.unravel_index(cells, shape)
    return np.ravel_multi_index((i, j, k), tuple(n - 1 for n in shape))


def test_all_valid_restatement_is_the_unmasked_one():
    g = np.random.RandomState(3).rand(7, 6, 9).astype(np.float32) * 2
    a = M.marching_cubes(g, 1.0, (-1, -1, -1), (1, 1, 1))
    b = R.marching_cubes_valid(g, np.ones(g.shape, bool), 1.0, (-1, -1, -1), (1, 1, 1))
    for x, z in zip(a, b):
        assert np.array_equal(x, z)
    v, f, n = R.marching_cubes_valid(g, np.zeros(g.shape, bool), 1.0, (-1, -1, -1), (1, 1, 1))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


# ---- argument checks of the new entry points: MVIP_EINVAL before any device work (the style of tests/test_abi_errors.py) -----------

def raw(name, *args):
    return getattr(_lib.load(), name)(*args)


def tsdf_args(**kw):
    a = dict(disp=P0, pose=P0, mask=P0, V=3, H=48, W=64, focal=60.0, nx=25, ny=19, nz=33, x0=-1.0, y0=-1.0, z0=-4.0, x1=1.0, y1=1.0,
             z1=-1.0, trunc=0.4, tsdf=P0, count=P0, stream=P0)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


INF, NAN = float('inf'), float('nan')
TSDF_BAD = [dict(nx=1), dict(ny=769), dict(nz=0), dict(nx=-5), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(V=-1),
            dict(x0=NAN), dict(y1=INF), dict(z0=-INF), dict(x0=1.0), dict(y0=2.0), dict(z1=-4.0), dict(focal=0.0), dict(focal=-1.0),
            dict(focal=INF), dict(focal=NAN), dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=INF), dict(trunc=NAN)]


@pytest.mark.parametrize('bad', TSDF_BAD, ids=[next(iter(b)) + '=' + str(next(iter(b.values()))) for b in TSDF_BAD])
def test_tsdf_fuse_rejects_bad_arguments(bad):
    args = tsdf_args(**bad)
    assert len(args) == len(_lib._SIGNATURES['mvip_tsdf_fuse'][1]), 'the case must follow the binding in _lib.py'
    assert raw('mvip_tsdf_fuse', *args) == EINVAL


def test_tsdf_fuse_rejects_null_operands():
    assert raw('mvip_tsdf_fuse', *tsdf_args()) == EINVAL
    assert raw('mvip_tsdf_fuse', *tsdf_args(V=0)) == EINVAL                              # V = 0 is legal, null outputs are not


def mc_args(**kw):
    a = dict(grid=P0, valid=P0, nx=8, ny=8, nz=8, iso=1.0, tri_table=P0, flags=P0, wg=P0, totals=P0, stream=P0)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


MC_BAD = [dict(nx=1), dict(ny=769), dict(nz=-1), dict(iso=0.0), dict(iso=-1.0), dict(iso=INF), dict(iso=NAN)]


@pytest.mark.parametrize('bad', MC_BAD + [{}], ids=[(next(iter(b)) + '=' + str(next(iter(b.values())))) if b else 'null' for b in MC_BAD + [{}]])
def test_mcubes_count_valid_rejects_bad_arguments(bad):
    args = mc_args(**bad)
    assert len(args) == len(_lib._SIGNATURES['mvip_mcubes_count_valid'][1]), 'the case must follow the binding in _lib.py'
    assert raw('mvip_mcubes_count_valid', *args) == EINVAL


def test_new_symbols_are_declared_and_the_abi_version_stays():
    assert 'mvip_tsdf_fuse' in _lib.DECLARED_SYMBOLS and 'mvip_mcubes_count_valid' in _lib.DECLARED_SYMBOLS
    assert _lib.ABI_VERSION == 5 and _lib.load().mvip_abi_version() == 5
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mvip_nerf.h')).read()
    assert 'int mvip_tsdf_fuse(' in header and 'int mvip_mcubes_count_valid(' in header
