"""The references of tests/test_hashgrid_model.py on their own (no GPU): the ODD lattice is exact in fp32 and its hashed
levels are no powers of two, the special rows reach the dense wrap, the gradient inputs keep every hidden pre-activation away
from 0 so that fp32 and fp64 take the same ReLU masks, and -- the evidence for MARGIN -- the fp32 oracle re-summed in permuted
pairs of k stays within MARGIN / 2 * E32 of the fp64 one for every output column and gradient tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradient_cases as G                               # noqa: E402
import hashgrid_model_cases as C                         # noqa: E402


@pytest.mark.parametrize('name', C.TABLES)
def test_lattice_tables(name):
    """Offsets are the running sum of the sizes; both tables have the dense levels 0-4 and 7, one with size == res^3 and one
    with size > res^3; every hashed level of ODD has a size that is a multiple of 8 and no power of two."""
    levels, n = C.lattice_levels(name)
    u = levels.view(np.uint32).astype(np.int64)
    assert list(u[:, 0].astype(np.uint32).view(np.float32)) == [float(s) for s in G.LATTICE_SCALES]
    assert list(u[:, 1]) == [s + 1 for s in G.LATTICE_SCALES]
    assert list(u[:, 2]) == list(np.concatenate([[0], np.cumsum(u[:-1, 3])])) and n == int(u[:, 3].sum())
    dense = C.dense_levels(levels)
    assert tuple(dense) == G.LATTICE_DENSE
    assert any(u[l, 3] == u[l, 1] ** 3 for l in dense) and any(u[l, 3] > u[l, 1] ** 3 for l in dense)
    hashed = [l for l in range(16) if l not in dense]
    pow2 = [bool(u[l, 3] & (u[l, 3] - 1) == 0) for l in hashed]
    assert all(u[l, 3] % 8 == 0 for l in hashed)
    assert all(pow2) if name == 'POW2' else not any(pow2)


@pytest.mark.parametrize('name', C.TABLES)
@pytest.mark.parametrize('n', [C.LATTICE_BASE, C.LATTICE_BIG])
def test_lattice_is_exact_in_fp32(name, n):
    """On the model lattice, out-of-box rows included: x, x * scale + 0.5 and the eight corner weights in fp32 equal their
    fp64 values, so fp32 cells are fp64 cells; the stored weights and table are float32, so they widen exactly."""
    inp = C.lattice_inputs(name, n)
    j = inp['j']
    assert (j[:4] == C.SPECIAL_J).all()
    oob = j[4:4 + C.N_OUT_OF_BOX]
    assert (((oob >= -16) & (oob <= -1)) | ((oob >= 129) & (oob <= 144))).all() and (oob < 0).any() and (oob > 128).any()
    assert ((j[20:] >= 0) & (j[20:] <= 128)).all()
    x64 = j.astype(np.float64) / 128.0
    x32 = x64.astype(np.float32)
    assert (x32.astype(np.float64) == x64).all()
    for s in G.LATTICE_SCALES:
        pos64 = x64 * s + 0.5
        pos32 = x32 * np.float32(s) + np.float32(0.5)
        assert pos32.dtype == np.float32 and (pos32.astype(np.float64) == pos64).all()
        assert ((x32 * np.float32(s)).astype(np.float64) == x64 * s).all()
        assert (np.floor(pos32).astype(np.int64) == np.floor(pos64).astype(np.int64)).all()
        w64, w32 = pos64 - np.floor(pos64), pos32 - np.floor(pos32)
        for k in range(8):
            f64 = [w64[:, d] if (k >> d) & 1 else 1.0 - w64[:, d] for d in range(3)]
            f32 = [w32[:, d] if (k >> d) & 1 else np.float32(1.0) - w32[:, d] for d in range(3)]
            p32 = f32[0] * f32[1] * f32[2]
            assert p32.dtype == np.float32 and (p32.astype(np.float64) == f64[0] * f64[1] * f64[2]).all()
    for key in ('table', 'sp', 'cp', 'dirs'):
        assert inp[key].dtype == np.float32
    assert inp['sp'].size == 3072 and inp['cp'].size == 7168
    a = (6.0 / 96) ** 0.5
    assert np.abs(inp['sp'][:2048]).max() <= a and np.abs(inp['sp'][:2048]).max() > 0.9 * a       # the model's Xavier rule


@pytest.mark.parametrize('name', C.TABLES)
def test_special_rows_reach_the_dense_wrap(name):
    """The face rows and all 16 out-of-box rows have a corner on a dense level whose index is at or beyond the level's size
    (hgf_corners' `idx %= size`); the interior vertex (64,64,64) at the origin-side rows does not have to."""
    levels, _ = C.lattice_levels(name)
    j = C.lattice_inputs(name, C.LATTICE_BASE)['j']
    hit = C.dense_wrap_rows(j, levels)
    print(f'{name}: {int(hit[:20].sum())} of the 20 special rows and {int(hit.sum())} of all {len(j)} rows reach the dense wrap')
    assert hit[0] and hit[3]                              # (128,128,128) and (64,0,128)
    assert hit[4:4 + C.N_OUT_OF_BOX].all()
    assert not hit[1]                                     # the origin: every corner index is below res^3
    assert hit[:C.NONFINITE_P].sum() >= 20


@pytest.mark.parametrize('name,n', [(t, C.LATTICE_BASE) for t in C.TABLES] + [('POW2', C.LATTICE_BIG)])
def test_lattice_permuted_pairs_within_half_margin(name, n):
    """oracle32 re-summed in permuted pairs of k against oracle64: every output column within MARGIN / 2 * E32, E32 > 0."""
    r64 = C.lattice_eval(name, n, torch.float64)
    _, E32, tol = C.lattice_reference(name, n)
    rp = C.lattice_eval(name, n, torch.float32, True)
    assert (E32 > 0).all() and (tol == C.MARGIN * E32).all()
    ratio = np.abs(rp - r64).max(0) / E32
    print(f'{name} n={n}: E32 {E32} at max|ref| {np.abs(r64).max(0)}; permuted pairs / E32 {ratio}')
    assert (ratio <= C.MARGIN / 2).all()
    assert (E32 < 1e-5 * np.abs(r64).max(0)).all()        # four orders below an O(1) error


def test_single_point_sample_is_no_tolerance():
    """Why small point counts use the 300-point case's E32: the error of one point is a single draw, and over the 300
    points the permuted-pair error of a point exceeds MARGIN times that point's own |oracle32 - oracle64| for some of them."""
    r64 = C.lattice_eval('POW2', C.LATTICE_BASE, torch.float64)
    e32 = np.abs(C.lattice_eval('POW2', C.LATTICE_BASE, torch.float32) - r64)
    ep = np.abs(C.lattice_eval('POW2', C.LATTICE_BASE, torch.float32, True) - r64)
    over = ep > C.MARGIN * e32
    print(f'{int(over.sum())} of {over.size} single-point values beyond MARGIN x their own fp32 error')
    assert over.any()


@pytest.mark.parametrize('P', C.MODULE_PS)
def test_module_inputs_and_relu_guard(P):
    """Fixed rows in place, ~10 % of the cotangent rows zero, every hidden pre-activation at least GUARD * max|z| of its layer
    from 0 in fp64, and the fp32 oracle's three ReLU masks equal the fp64 oracle's."""
    inp = C.module_inputs(P)
    fixed = C.module_fixed_rows()
    assert len(fixed) == 18 and (inp['x'][:18] == fixed).all() and (np.abs(inp['x'][18:]) <= 4).all()
    dead = (inp['g'] == 0).all(-1)
    assert (dead == (inp['g'] == 0).any(-1)).all() and 0.05 < dead.mean() < 0.15 and not dead[:18].any()
    r64, r32 = C.module_eval(P, torch.float64), C.module_eval(P, torch.float32)
    print(f'P={P}: smallest |z| / (GUARD max|z|) {r64["zmargin"].min():.3g} (fixed rows {r64["zmargin"][:18].min():.3g})')
    assert (r64['zmargin'] >= 1.0).all()
    for a, b in zip(r64['masks'], r32['masks']):
        assert a.shape == (P, 64) and (a == b).all()
        assert 0.2 < a.mean() < 0.8
    levels = C.module_model().levels.numpy()
    assert C.dense_levels(levels) == [0, 1, 2]


@pytest.mark.parametrize('P', C.MODULE_PS)
def test_module_permuted_pairs_within_half_margin(P):
    """The module case: outputs and all six parameter gradients of the permuted-pair fp32 evaluation within MARGIN / 2 * E32
    of fp64 autograd; E32 > 0 everywhere; table entries no live point touches are exactly 0 in every evaluation."""
    r64, E32 = C.module_reference(P)
    rp = C.module_eval(P, torch.float32, True)
    ratios = {'out': np.abs(rp['out'] - r64['out']).max(0) / E32['out']}
    for name in C.GRAD_NAMES:
        assert E32[name] > 0
        ratios[name] = float(np.abs(rp[name] - r64[name]).max() / E32[name])
        assert E32[name] < 1e-5 * np.abs(r64[name]).max()
    assert (E32['out'] > 0).all()
    print(f'P={P}: E32 {E32}; permuted pairs / E32 {ratios}')
    assert (ratios['out'] <= C.MARGIN / 2).all()
    assert all(ratios[name] <= C.MARGIN / 2 for name in C.GRAD_NAMES)
    touched = C.module_touched(P)
    assert touched.any() and not touched.all()
    for r in (r64, rp, C.module_eval(P, torch.float32)):
        assert r['table'].shape == (len(touched), 2) and (r['table'][~touched] == 0).all()
    assert (r64['table'][touched] != 0).mean() > 0.9


def test_sh4_reference():
    """Row 0 is the float32 constant in both precisions (E32 = 0: compared for equality); every other row has E32 > 0."""
    d = C.sh_inputs()
    r64, E32 = C.sh_reference()
    assert d.shape == (C.SH_BASE, 3) and r64.shape == (C.SH_BASE, 16)
    assert E32[0] < 2.0 ** -25 and (E32[1:] > 0).all() and (E32[1:] < 1e-6).all()
    assert np.float64(C.SH_ROW0) == np.float64(np.float32(r64[0, 0]))
    np.testing.assert_allclose(r64[0, 1:4], [0, 0, -0.48860251190291987], atol=1e-15)      # +x axis
    assert max(C.SH_PS) == C.SH_BASE
