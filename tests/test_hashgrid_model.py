"""The hash-grid model NeRF_TCNN against the published algorithm in fp64 at EVERY point, forward and all parameter gradients
(inputs, references and the tolerance rule: tests/hashgrid_model_cases.py; the references alone: tests/test_hashgrid_model_cpu.py).
  fused kernel   csrc/hashgrid_fused.hip on lattices that are exact in fp32: both table kinds (hashed levels of power-of-two
                 and of other sizes), faces, out-of-box points, ragged tiles, the persistent loop; non-finite inputs stay local
  module         NeRF_TCNN on its own table at bound = 100: the fused, the unfused no-grad and the grad-enabled forward against
                 one reference; the gradients of sigma_net.params, color_net.params and encoder.params against fp64 autograd
  sh4            csrc/hashgrid.hip::sh4_kernel
Every element is compared with MARGIN * E32 of its output column or gradient tensor, E32 = max |fp32 oracle - fp64 oracle|.
Each test prints its largest error as a share of that tolerance before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashgrid_model_cases as C                         # noqa: E402

pytestmark = pytest.mark.gpu


def T(x, dev):
    return torch.tensor(np.asarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def _fused_lattice(cuda, name, P, bound=0.0, x=None, dirs=None):
    """ops.hashgrid_mlp_pack + ops.hashgrid_nerf_forward on the first P rows of the lattice case, level table passed directly."""
    from mvip_nerf_amd import ops
    inp = C.lattice_inputs(name, C.lattice_base(P))
    if x is None:
        jf = inp['j'][:P].astype(np.float32)
        x = jf / np.float32(128.0) if bound == 0.0 else np.float32(-bound) + jf / np.float32(16.0)
    if dirs is None:
        dirs = inp['dirs'][:P]
    img = ops.hashgrid_mlp_pack(T(inp['sp'], cuda), T(inp['cp'], cuda))
    out = ops.hashgrid_nerf_forward(T(x, cuda), T(dirs, cuda), T(inp['table'].reshape(-1), cuda), T(inp['levels'], cuda), img,
                                    bound)
    assert out.shape == (P, 4) and out.dtype == torch.float32
    return out


def _assert_columns(got, ref, tol, what):
    """every element of got [P,C] within tol [C] of ref; prints the worst share of the tolerance first."""
    err = np.abs(got.astype(np.float64) - ref)
    share = C.worst_ratio(got, ref, tol[None, :])
    print(f'{what}: worst error {err.max():.3g} at max|ref| = {np.abs(ref).max():.3g}, {share:.3g} of the tolerance '
          f'(MARGIN {C.MARGIN} x E32 {tol / C.MARGIN})')
    bad = ~(err <= tol[None, :])
    assert not bad.any(), (f'{what}: {int(bad.sum())} values outside the tolerance, rows {np.nonzero(bad.any(1))[0][:20]}, '
                           f'columns {np.nonzero(bad.any(0))[0]}, worst {err.max():.3g}')


@pytest.mark.parametrize('name,P', [('POW2', P) for P in C.LATTICE_PS] + [('ODD', P) for P in C.LATTICE_PS[:-1]])
def test_fused_kernel_on_lattice_vs_fp64(cuda, name, P):
    """hgf_pack_kernel + hgf_forward_kernel on the integer-scale lattice against the fp64 oracle: all four outputs of every
    point -- the faces, (64,64,64), 16 out-of-box rows (uint32 wrap-around cells) -- within MARGIN * E32 of their column.
    POW2: hashed levels masked; ODD: hashed levels of size 4104 / 65544 / 131080 (`hsh % size`).  P = 1, 31, 32, 33: one and
    two ragged tiles; 300; 65573: a second sweep of the persistent loop ending on a ragged tile (POW2 only).  bound = 4 with
    x' = -4 + j/16 equals the bound = 0 call bit for bit, and so does a repeated call.
    Measured on the MI355X: worst error 3.7e-8 .. 4.3e-7 at max|ref| = 0.16 .. 2.3; 0.04 - 0.21 of the tolerance over the eleven
    cases (0.21 at POW2 P = 65573, 0.15 at ODD P = 300)."""
    ref, _, tol = C.lattice_reference(name, P)
    out = _fused_lattice(cuda, name, P)
    _assert_columns(N(out), ref, tol, f'fused lattice {name} P={P}')
    assert torch.equal(bits(out), bits(_fused_lattice(cuda, name, P))), 'a repeated call differs'
    assert torch.equal(bits(out), bits(_fused_lattice(cuda, name, P, bound=4.0))), 'bound = 4 differs from bound = 0'


@pytest.mark.parametrize('name', C.TABLES)
def test_fused_kernel_nonfinite_points_stay_local(cuda, name):
    """P = 70: one point's position, then one component of its direction, replaced by NaN, +Inf and -Inf -- the other 69
    points' outputs are bit-identical to the all-finite run.  (Every index of hgf_corners is reduced below the level's size:
    `idx %= size`, `hsh & mask` or `hsh % size`, whatever the cell; a float-to-int conversion of NaN / Inf saturates.)
    Nothing is asserted about the replaced point's own outputs.
    Measured on the MI355X: bit-identical in all twelve runs; the all-finite run at 0.13 of the tolerance."""
    P, row = C.NONFINITE_P, C.NONFINITE_ROW
    inp = C.lattice_inputs(name, C.LATTICE_BASE)
    x = (inp['j'][:P].astype(np.float32) / np.float32(128.0))
    dirs = inp['dirs'][:P].copy()
    base = _fused_lattice(cuda, name, P, x=x, dirs=dirs)
    ref, _, tol = C.lattice_reference(name, P)
    _assert_columns(N(base), ref, tol, f'non-finite base {name}')
    others = torch.arange(P, device=cuda) != row
    for value in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[row] = value
        db = dirs.copy()
        db[row, 1] = value
        for what, got in (('position', _fused_lattice(cuda, name, P, x=xb, dirs=dirs)),
                          ('direction', _fused_lattice(cuda, name, P, x=x, dirs=db))):
            same = torch.equal(bits(got)[others], bits(base)[others])
            print(f'non-finite {name}: {what} = {value}: other points bit-identical: {same}')
            assert same, f'{what} = {value} at point {row} changed another point'


def _module(cuda):
    """A copy of the case's CPU module on the GPU (same parameter values)."""
    import copy
    return copy.deepcopy(C.module_model()).to(cuda)


@pytest.mark.parametrize('P', C.MODULE_PS)
def test_module_forward_routes_vs_fp64(cuda, P):
    """NeRF_TCNN on its own table, bound = 100: scene-scale points, the six face centres, the eight corners at +-100, points
    at +-99.99.  The reference forms the positions in fp32 as hg_cell does and is fp64 after that, so a point in another cell
    fails by O(1).  Every point of the fused no-grad forward, the unfused no-grad forward and the grad-enabled forward within
    MARGIN * E32 of its column.
    Measured on the MI355X: fused 0.19 (P = 300) and 0.13 (P = 4389) of the tolerance, unfused and grad-enabled 0.125 at both
    (their worst element equals the fp32 oracle's); worst error 1.6e-7 .. 2.6e-7 at max|ref| = 0.7 .. 0.84."""
    r64, E32 = C.module_reference(P)
    inp = C.module_inputs(P)
    net = _module(cuda)
    x = T(np.concatenate([inp['x'], inp['dirs']], -1), cuda)
    with torch.no_grad():
        assert net.fused_inference
        fused = net(x)
        net.fused_inference = False
        plain = net(x)
    net.fused_inference = True
    train = net(x)
    assert train.requires_grad and not fused.requires_grad and not plain.requires_grad
    for what, got in (('fused', fused), ('unfused', plain), ('grad-enabled', train)):
        assert got.shape == (P, 4)
        _assert_columns(N(got), r64['out'], C.MARGIN * E32['out'], f'module P={P} {what} forward')


@pytest.mark.parametrize('P', C.MODULE_PS)
def test_module_parameter_gradients_vs_fp64_autograd(cuda, P):
    """loss = (out * g).sum() with all four cotangents zero on ~10 % of the points, inputs kept GUARD away from every ReLU
    kink: the gradients of sigma_net.params (W1, W2), color_net.params (C1, C2, C3) and encoder.params through the model --
    skinny_wgrad_kernel on zero-padded ragged point counts, skinny_fwd_kernel's data gradients, hg_backward_kernel<false> --
    element by element within MARGIN * E32 of their tensor; table entries nothing contributes to exactly 0.
    Measured on the MI355X, share of the tolerance: P = 300: W1 0.07, W2 0.11, C1 0.15, C2 0.11, C3 0.10, table 0.28;
    P = 4389: W1 0.11, W2 0.07, C1 0.09, C2 0.11, C3 0.09, table 0.07 (E32 = 1.8e-7 .. 5.8e-7 of max|grad|; the order of the
    table's atomics varies run to run)."""
    r64, E32 = C.module_reference(P)
    inp = C.module_inputs(P)
    net = _module(cuda)
    assert net.table_grad_atomics == 'float32'
    out = net(T(np.concatenate([inp['x'], inp['dirs']], -1), cuda))
    (out * T(inp['g'], cuda)).sum().backward()
    gs, gc = N(net.sigma_net.params.grad), N(net.color_net.params.grad)
    got = dict(zip(C.GRAD_NAMES[:5], C.matrices(torch.from_numpy(gs), torch.from_numpy(gc))))
    got = {k: v.numpy() for k, v in got.items()}
    got['table'] = N(net.encoder.params.grad).reshape(-1, 2)
    shares = {k: C.worst_ratio(got[k], r64[k], C.MARGIN * E32[k]) for k in C.GRAD_NAMES}
    print(f'module P={P} gradients, worst share of the tolerance: ' + ', '.join(f'{k} {v:.3g}' for k, v in shares.items())
          + '; E32 / max|grad|: ' + ', '.join(f'{k} {E32[k] / np.abs(r64[k]).max():.3g}' for k in C.GRAD_NAMES))
    touched = C.module_touched(P)
    assert (got['table'][~touched] == 0).all(), 'entries without a contribution must stay exactly 0'
    for k in C.GRAD_NAMES:
        assert got[k].shape == r64[k].shape
        bad = ~(np.abs(got[k].astype(np.float64) - r64[k]) <= C.MARGIN * E32[k])
        assert not bad.any(), f'd{k}: {int(bad.sum())} of {bad.size} elements outside the tolerance ({shares[k]:.3g} of it)'


@pytest.mark.parametrize('P', C.SH_PS)
def test_sh4_kernel_vs_fp64(cuda, P):
    """sh4_kernel on +-axes, (1,1,1)/sqrt(3), non-unit and zero vectors and random unit vectors against the fp64 basis: rows
    1-15 within MARGIN * E32 of their row, row 0 equal to the float32 constant.  P = 1; 255, 256, 257: around one block.
    Measured on the MI355X: 0.025 of the tolerance at P = 1, 0.125 at the others (worst error 2.5e-7 at max|ref| = 6.5: the
    kernel's worst element equals the fp32 oracle's)."""
    from mvip_nerf_amd import ops
    r64, E32 = C.sh_reference()
    got = N(ops.sh4(T(C.sh_inputs()[:P], cuda)))
    assert got.shape == (16, P) and got.dtype == np.float32
    assert (got[0] == C.SH_ROW0).all()
    _assert_columns(got.T[:, 1:], r64[:P, 1:], C.MARGIN * E32[1:], f'sh4 P={P}')
