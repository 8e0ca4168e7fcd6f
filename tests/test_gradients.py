"""The gradient kernels against fp64 autograd through the oracle, at every dispatch width and on the shapes where they
can go wrong (inputs, references and bounds: tests/gradient_cases.py; the references alone: tests/test_gradients_cpu.py).
  compositing   csrc/composite.hip, ITEMS = 1 / 2 / 4 / 8, every flag combination, every subset of output cotangents
  plane fit     csrc/normal_fit.hip, windows clipped on all sides, H or W = 1, several blocks; depth2xyz; the chain
  hash grid     csrc/hashgrid.hip on a lattice that is exact in fp32: every level, hashed ones included, entry by entry
Each test prints its largest error against the bound before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradient_cases as C                               # noqa: E402

pytestmark = pytest.mark.gpu


def T(x, dev):
    return torch.tensor(np.asarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nanmax(r))


# ---------------------------------------------------------------------------------------------- compositing
def _composite_case(cuda, S, B, white, detach, use_noise, subset):
    from mvip_nerf_amd import ops
    inp = C.composite_inputs(S, B)
    o_ref, g_ref = C.composite_reference(S, B, white, detach, use_noise, subset)
    raw = T(inp['raw'], cuda).requires_grad_(True)
    need_alpha = 'alpha' in subset                       # without it the function has five outputs: g_alpha is never passed
    out = ops.composite(raw, T(inp['z'], cuda), T(inp['rows'], cuda), T(inp['noise'], cuda) if use_noise else None,
                        white_bkgd=white, detach_weights=detach, need_alpha=need_alpha)
    outs = dict(zip(C.COMPOSITE_OUTPUTS, out))
    tag = f'S={S} B={B} white={white} detach={detach} noise={use_noise} loss={"+".join(subset)}'
    fwd = 0.0
    for name, val in outs.items():
        if val is None:
            assert name == 'alpha' and not need_alpha
            continue
        fwd = max(fwd, worst_ratio(N(val), o_ref[name], C.COMPOSITE_FWD_ATOL + C.COMPOSITE_FWD_RTOL * np.abs(o_ref[name])))
        np.testing.assert_allclose(N(val), o_ref[name], rtol=C.COMPOSITE_FWD_RTOL, atol=C.COMPOSITE_FWD_ATOL, equal_nan=True,
                                   err_msg=f'{name}: {tag}')
    C.composite_loss(outs, {k: T(inp['g_' + k], cuda) for k in subset}, subset).backward()
    d_raw = N(raw.grad)
    scale = np.nanmax(np.abs(g_ref))
    np.testing.assert_array_equal(np.isnan(d_raw), np.isnan(g_ref), err_msg=f'd_raw NaN pattern: {tag}')
    bwd = worst_ratio(d_raw, g_ref, C.COMPOSITE_ATOL * scale + C.COMPOSITE_RTOL * np.abs(g_ref))
    err = float(np.nanmax(np.abs(d_raw - g_ref)) / scale)
    np.testing.assert_allclose(d_raw, g_ref, rtol=C.COMPOSITE_RTOL, atol=C.COMPOSITE_ATOL * scale, equal_nan=True,
                               err_msg=f'd_raw: {tag}')
    return fwd, bwd, err


@pytest.mark.parametrize('S', C.COMPOSITE_S)
def test_composite_backward_vs_fp64_autograd(cuda, S):
    """composite_bwd_kernel<ITEMS> against torch autograd through raw2outputs in fp64, B = 19 (not a multiple of the four
    rays per workgroup; the fixed rows of gradient_cases.composite_inputs included): d_raw at test_composite_golden's
    tolerance (rtol 2e-4, atol 2e-6 nanmax|d_raw_ref|), the outputs of the same calls at test_composite_vs_oracle_sizes'
    (3e-5 / 3e-6).  Every flag combination with cotangents on all six outputs (alpha included); then each smaller set of
    outputs in the loss, so that autograd hands the kernel None -- a null pointer -- for the others.
    Measured on the MI355X: d_raw <= 4.8e-7 nanmax|d_raw_ref| for S >= 7 (<= 0.22 of the tolerance); 1.9e-6 (0.95 of it) at S = 2
    with the loss on disp alone, on a ray whose whole weight (acc = 0.04) sits on its first sample -- the true gradient there is
    exactly 0 and what is left is the rounding of q = depth / acc times gq / acc (no fp32 evaluation of q does better; the kernel
    forms (gq / acc) (z - q) from the difference for that reason).  Forward <= 0.02 of its tolerance."""
    worst = (0.0, 0.0, 0.0)
    for white, detach, use_noise, subset in C.composite_cases(S):
        worst = tuple(max(a, b) for a, b in zip(worst, _composite_case(cuda, S, 19, white, detach, use_noise, subset)))
    print(f'composite S={S} (ITEMS={C.composite_items(S)}): forward {worst[0]:.3g} of its tolerance, d_raw {worst[1]:.3g} of its '
          f'tolerance, max |d_raw - ref| = {worst[2]:.3g} nanmax|d_raw_ref|')


def test_composite_backward_single_ray(cuda):
    """B = 1: three of the workgroup's four waves have no ray."""
    white, detach, use_noise, subset = C.composite_cases(130)[0]
    fwd, bwd, err = _composite_case(cuda, 130, 1, white, detach, use_noise, subset)
    print(f'composite S=130 B=1: forward {fwd:.3g} of its tolerance, d_raw {bwd:.3g} of its tolerance ({err:.3g} nanmax|d_raw_ref|)')


# ---------------------------------------------------------------------------------------------- plane fit
@pytest.mark.parametrize('H,W,k', C.NORMAL_SHAPES)
def test_normal_fit_backward_shapes(cuda, H, W, k):
    """normal_fit forward and d_points (normal_bwd_sums_kernel, box_rows_kernel<false>, normal_bwd_points_kernel) against
    the box-sum algebra in fp64 with autograd, on point clouds whose window moment matrices have condition <= 1e3
    (asserted in test_gradients_cpu.py): normals at test_normal_fit_shapes' tolerance (rtol 5e-4, atol 5e-5 max|ref|),
    d_points at test_normal_fit_golden's gradient tolerance (rtol 2e-3, atol 2e-4 max|grad_ref|).
    Measured on the MI355X: normals <= 1.2e-6 max|n|, d_points <= 1.1e-6 max|grad| (<= 0.006 of either tolerance)."""
    from mvip_nerf_amd import ops
    pts, g = C.normal_inputs(H, W)
    n_ref, d_ref = C.normal_reference(H, W, k)
    p = T(pts, cuda).requires_grad_(True)
    n = ops.normal_fit(p, k)
    (n * T(g, cuda)).sum().backward()
    ns, ds = np.abs(n_ref).max(), np.abs(d_ref).max()
    print(f'normal_fit {H}x{W} k={k}: normals {np.abs(N(n) - n_ref).max() / ns:.3g} max|n|, '
          f'{worst_ratio(N(n), n_ref, C.NORMAL_FWD_ATOL * ns + C.NORMAL_FWD_RTOL * np.abs(n_ref)):.3g} of the tolerance; d_points '
          f'{np.abs(N(p.grad) - d_ref).max() / ds:.3g} max|grad|, '
          f'{worst_ratio(N(p.grad), d_ref, C.NORMAL_BWD_ATOL * ds + C.NORMAL_BWD_RTOL * np.abs(d_ref)):.3g} of the tolerance')
    np.testing.assert_allclose(N(n), n_ref, rtol=C.NORMAL_FWD_RTOL, atol=C.NORMAL_FWD_ATOL * ns, err_msg='normals')
    np.testing.assert_allclose(N(p.grad), d_ref, rtol=C.NORMAL_BWD_RTOL, atol=C.NORMAL_BWD_ATOL * ds, err_msg='d_points')


@pytest.mark.parametrize('H,W', C.DEPTH_SHAPES)
def test_depth2xyz_backward_shapes(cuda, H, W):
    """ops.depth2xyz with fx != fy and an off-centre, non-integer principal point: points at test_normal_fit_golden's
    tolerance (1e-6 / 1e-7), d_depth against fp64 autograd within 4 u (|g_x (w - cx) / fx| + |g_y (h - cy) / fy| + |g_z|)
    per pixel.  Measured on the MI355X: points <= 0.13 of the tolerance, d_depth <= 0.59 of the bound."""
    from mvip_nerf_amd import ops
    depth, K, g = C.depth_inputs(H, W)
    p_ref, d_ref = C.depth_reference(H, W)
    d = T(depth, cuda).requires_grad_(True)
    pts = ops.depth2xyz(d, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    assert pts.shape == (H, W, 3)
    (pts * T(g, cuda)).sum().backward()
    bound = C.depth_grad_bound(H, W)
    print(f'depth2xyz {H}x{W}: points {worst_ratio(N(pts), p_ref, 1e-7 + 1e-6 * np.abs(p_ref)):.3g} of the tolerance, '
          f'd_depth {worst_ratio(N(d.grad), d_ref, bound):.3g} of the bound')
    np.testing.assert_allclose(N(pts), p_ref, rtol=1e-6, atol=1e-7, err_msg='points')
    assert (np.abs(N(d.grad).astype(np.float64) - d_ref) <= bound).all(), 'd_depth'


def test_depth_to_normals_chain(cuda):
    """depth -> ops.depth2xyz -> transpose -> ops.normal_fit -> loss at 9x64, k = 5, against the same chain in fp64: the two
    autograd functions together outside the golden frame.  Tolerances as in test_normal_fit_backward_shapes (the gradient's
    is the one test_normal_fit_golden applies to this very chain); test_gradients_cpu.py asserts the conditioning of
    these points and that the fp32 storage of the box sums alone stays under half of each tolerance.
    Measured on the MI355X: normals 5.2e-5 max|n| (0.35 of the tolerance), d_depth 3.2e-5 max|grad| (0.06)."""
    from mvip_nerf_amd import ops
    depth, K, g = C.chain_inputs()
    p_ref, n_ref, d_ref = C.chain_reference()
    d = T(depth, cuda).requires_grad_(True)
    pts = ops.depth2xyz(d, K[0, 0], K[1, 1], K[0, 2], K[1, 2]).permute(2, 0, 1)
    n = ops.normal_fit(pts, C.CHAIN_SHAPE[2])
    (n * T(g, cuda)).sum().backward()
    ns, ds = np.abs(n_ref).max(), np.abs(d_ref).max()
    print(f'chain: normals {np.abs(N(n) - n_ref).max() / ns:.3g} max|n|, '
          f'{worst_ratio(N(n), n_ref, C.NORMAL_FWD_ATOL * ns + C.NORMAL_FWD_RTOL * np.abs(n_ref)):.3g} of the tolerance; d_depth '
          f'{np.abs(N(d.grad) - d_ref).max() / ds:.3g} max|grad|, '
          f'{worst_ratio(N(d.grad), d_ref, C.NORMAL_BWD_ATOL * ds + C.NORMAL_BWD_RTOL * np.abs(d_ref)):.3g} of the tolerance')
    np.testing.assert_allclose(N(pts), p_ref, rtol=1e-6, atol=1e-7, err_msg='points')
    np.testing.assert_allclose(N(n), n_ref, rtol=C.NORMAL_FWD_RTOL, atol=C.NORMAL_FWD_ATOL * ns, err_msg='normals')
    np.testing.assert_allclose(N(d.grad), d_ref, rtol=C.NORMAL_BWD_RTOL, atol=C.NORMAL_BWD_ATOL * ds, err_msg='d_depth')


# ---------------------------------------------------------------------------------------------- hash grid
def _lattice_run(cuda, P, half2=False, bound=0.0):
    from mvip_nerf_amd import ops
    levels, j, table, dout, _ = C.lattice_inputs(P)
    jf = j.astype(np.float32)
    x = jf / np.float32(128.0) if bound == 0.0 else np.float32(-bound) + jf / np.float32(16.0)
    t = T(table.reshape(-1), cuda).requires_grad_(True)
    f = ops.hashgrid_encode(T(x, cuda), t, T(levels, cuda), bound, half2)
    assert f.shape == (32, P)
    return f, t, dout


@pytest.mark.parametrize('P', [C.LATTICE_P, C.LATTICE_P_SMALL])
def test_hashgrid_exact_lattice_vs_fp64(cuda, P):
    """hg_forward_kernel and hg_backward_kernel<false> on the integer-scale lattice (positions and corner weights exact in
    fp32, test_gradients_cpu.py) against the fp64 oracle, all 16 levels, the hashed ones included:
      features        |got - ref| <= 8 u sum_k |w_k t_k| + u |ref|, all 32 rows
      table gradient  |got - ref| <= (n_e + 2) u A_e entry by entry (n_e contributions, A_e = sum |w g| over them);
                      exactly 0 where nothing contributes
    with dout zero on both feature rows of ~10 % of the (level, point) pairs (the kernel's skip).  P = 4389: two backward
    tiles, a ragged last tile, a ragged last 256-block; P = 300: a single partial tile.
    Measured on the MI355X: features 4.1e-7 at max|f| = 2.8 (0.45 of the bound), table gradient <= 0.47 of the bound, 3.2 - 3.6 u A_e
    worst (the order of the atomics varies run to run)."""
    ref = C.lattice_reference(P)
    f, t, dout = _lattice_run(cuda, P)
    fb, gb = C.lattice_forward_bound(ref), C.lattice_backward_bound(ref)
    f.backward(T(dout, cuda))
    grad = N(t.grad).reshape(-1, 2).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        in_A = np.nanmax(np.where(ref['A'] > 0, np.abs(grad - ref['grad']) / ref['A'], 0.0)) / C.U
    print(f'hashgrid lattice P={P}: features {np.abs(N(f) - ref["f"]).max():.3g} at max|f| = {np.abs(ref["f"]).max():.3g}, '
          f'{worst_ratio(N(f), ref["f"], fb):.3g} of the bound; table gradient {worst_ratio(grad, ref["grad"], gb):.3g} of the bound, '
          f'{in_A:.3g} u A_e worst')
    bad = np.abs(N(f).astype(np.float64) - ref['f']) > fb
    assert not bad.any(), f'features: {int(bad.sum())} outside the bound, feature rows {sorted(set(np.nonzero(bad)[0]))}'
    none = ref['count'] == 0
    assert none.any() and (grad[none] == 0).all(), 'entries without a contribution must stay exactly 0'
    bad = np.abs(grad - ref['grad']) > gb
    off = C.lattice_levels()[0].view(np.uint32)[:, 2]
    lv = sorted(set(int(np.searchsorted(off, e, side='right')) - 1 for e in np.nonzero(bad)[0]))
    assert not bad.any(), f'table gradient: {int(bad.sum())} values outside the bound, levels {lv}'


def test_hashgrid_bound_transform_is_bit_identical(cuda):
    """bound = 4 with x' = -4 + j/16: (x' + 4) / 8 = j/128 exactly, so the features equal the bound = 0 call's bit for bit."""
    f0, _, _ = _lattice_run(cuda, C.LATTICE_P)
    f4, _, _ = _lattice_run(cuda, C.LATTICE_P, bound=4.0)
    assert torch.equal(f0.view(torch.int32), f4.view(torch.int32))


def test_hashgrid_half2_lattice_vs_fp64(cuda):
    """hg_backward_kernel<true> (half-pair atomics for the contributions that miss the LDS map) on the lattice against the
    fp64 table gradient, held to what test_half2_table_gradient_option claims for the mode: finite, relative L2 error
    < 1e-2 over the whole table and over the scattered levels (12 and up) on their own.  Measured on the MI355X: 8.9e-5 for both."""
    ref = C.lattice_reference(C.LATTICE_P)
    f, t, dout = _lattice_run(cuda, C.LATTICE_P, half2=True)
    f.backward(T(dout, cuda))
    grad = N(t.grad).reshape(-1, 2).astype(np.float64)
    assert np.isfinite(grad).all()
    fine = int(C.lattice_levels()[0].view(np.uint32)[12, 2])
    rel = np.linalg.norm(grad - ref['grad']) / np.linalg.norm(ref['grad'])
    rel_fine = np.linalg.norm(grad[fine:] - ref['grad'][fine:]) / np.linalg.norm(ref['grad'][fine:])
    print(f'hashgrid half2 lattice: relative L2 error {rel:.3g} (levels >= 12: {rel_fine:.3g})')
    assert rel < 1e-2 and rel_fine < 1e-2, (rel, rel_fine)
