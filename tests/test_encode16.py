"""The input encoding of the 16-points-per-wave kernels, evaluated once per wave (csrc/mlp_device16.h, encode16_wave):

  * the probe entry mvip_mlp_encode16_probe runs the per-channel route (one sinf or cosf per fragment channel and lane) and
    the once-per-wave route (one sincosf per distinct argument, staged through LDS) on the same inputs: equal bit for bit;
  * the network outputs of every kernel that encodes this way, and a two-launch render, equal bit for bit what the commit
    before the change computed (tests/golden/encode16_parent.npz, written by tools/gen_encode16_golden.py from
    record_outputs() below -- the forward kernels have no atomics, so the record is deterministic).
"""
import os
import types

import numpy as np
import pytest
import torch

from oracle.weights import seeded_state_dict, bench_like_rays

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encode16_parent.npz')
P_POINTS = 4099                     # 32 workgroups of 128 points and 3 more: the last workgroup is partial, with dead lanes


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


# ---- 1: the probe ----------------------------------------------------------------------------------------------------

def probe_inputs(P, seed):
    """[P, 3] points and directions: uniform in [-8, 8], directions alternately normalised and not; from P = 129 on every
    special class of value is planted at fixed places (P = 1 gets them from special_single_points)."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-8., 8., size=(P, 3)).astype(np.float32)
    dirs = rs.uniform(-8., 8., size=(P, 3)).astype(np.float32)
    unit = dirs / np.linalg.norm(dirs.astype(np.float64), axis=-1, keepdims=True)
    dirs[0::2] = unit[0::2].astype(np.float32)
    special = np.array([0., -0., 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 1e5, -1e5, 1e8, -1e8, np.inf, -np.inf, np.nan,
                        8., -8., 3.1415927, 1.5707964, 7.9999995], dtype=np.float32)
    flat_p, flat_d = pts.reshape(-1), dirs.reshape(-1)
    if P == 1:
        return pts, dirs
    for k, v in enumerate(special):
        flat_p[(7 * k + 3) % flat_p.size] = v
        flat_d[(11 * k + 5) % flat_d.size] = v
    return pts, dirs


def special_single_points():
    """One-point inputs (P = 1): every special value in every axis of the point and of the direction."""
    vals = [0., -0., 1e-45, -5.9e-39, 1e5, -1e8, np.inf, -np.inf, np.nan, 0.37]
    out = []
    for k, v in enumerate(vals):
        p = np.array([[0.25, -1.5, 3.0]], dtype=np.float32)
        d = np.array([[0.6, 0., -0.8]], dtype=np.float32)
        p[0, k % 3] = v
        d[0, (k + 1) % 3] = v
        out.append((p, d))
    return out


def run_probe(pts, dirs, dev):
    from mvip_nerf_amd._lib import ptr, stream, call
    P = pts.shape[0]
    tp, td = T(pts, dev), T(dirs, dev)
    old = torch.full((P, 96), 7.25, device=dev)
    new = torch.full((P, 96), -7.25, device=dev)
    call('mvip_mlp_encode16_probe', ptr(tp), ptr(td), P, ptr(old), ptr(new), stream())
    torch.cuda.synchronize()
    return N(old), N(new)


def channel_reference(x3, n_oct, width):
    """fp64 encoding of fp32 coordinates [P, 3] in Embedder order, zero padded to `width` channels; the argument x * 2^o is
    exact in fp32 (a power-of-two scale), so fp64 sin / cos of it is the exact target."""
    x = x3.astype(np.float64)
    cols = [x]
    for o in range(n_oct):
        cols += [np.sin(x * 2. ** o), np.cos(x * 2. ** o)]
    e = np.concatenate(cols, -1)
    return np.concatenate([e, np.zeros((x.shape[0], width - e.shape[1]))], -1)


def check_probe(pts, dirs, dev):
    old, new = run_probe(pts, dirs, dev)
    nan_old, nan_new = np.isnan(old), np.isnan(new)
    np.testing.assert_array_equal(nan_old, nan_new)
    a, b = old.view(np.int32), new.view(np.int32)
    mism = (a != b) & ~nan_old
    print('P', pts.shape[0], 'channels differing in bits:', int(mism.sum()), 'NaN channels:', int(nan_old.sum()))
    assert not mism.any(), np.argwhere(mism)[:8]
    with np.errstate(invalid='ignore'):
        ref = np.concatenate([channel_reference(pts, 10, 64), channel_reference(dirs, 4, 32)], -1)
        small = np.concatenate([np.repeat((np.abs(pts) <= 8.)[:, None, :], 21, 1).reshape(-1, 63),
                                np.zeros((pts.shape[0], 1), bool),
                                np.repeat((np.abs(dirs) <= 8.)[:, None, :], 9, 1).reshape(-1, 27),
                                np.zeros((pts.shape[0], 5), bool)], -1)
        # the identity channels are exact; |sin|, |cos| <= 1 carry at most half an ulp of 1 = 6e-8 plus the reduction's error
        err = np.abs(new.astype(np.float64) - ref)[small]
    print('max |new - fp64| over finite |x| <= 8:', float(err.max()) if err.size else 0.)
    assert (err <= 1e-7).all()
    # the padding is zero whatever the inputs
    assert (new[:, 63] == 0).all() and (new[:, 64 + 27:] == 0).all()
    return new


@pytest.mark.parametrize('P', [1, 129, 4099])
def test_probe_routes_agree_bitwise(cuda, P):
    """Old route == new route as bit patterns (NaN positions equal as NaN), and within 1e-7 of fp64 for finite |x| <= 8."""
    pts, dirs = probe_inputs(P, seed=P)
    check_probe(pts, dirs, cuda)
    if P == 1:
        for p, d in special_single_points():
            check_probe(p, d, cuda)


# ---- 2: network outputs against the commit before the change ----------------------------------------------------------

def make_args(**kw):
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=64, alpha_model_path=None,
             netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=3e-3,
             basedir='/tmp/mvip_test', expname='none', ft_path=None, no_reload=True, perturb=1., N_samples=64,
             white_bkgd=True, raw_noise_std=1., dataset_type='llff', no_ndc=True, lindisp=True, sigma_loss=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def stash_sums(stash, P):
    """Two int64 checksums per row tile of the stash ([row tile][point tile of 32][32][32] fp32, point tiles in whole
    workgroups of 128 points): the sum of the bit patterns and the sum weighted by position."""
    b = stash.view(torch.int32).to(torch.int64).reshape(-1, (P + 127) // 128 * 4 * 1024)
    w = (torch.arange(b.shape[1], device=b.device, dtype=torch.int64) % 65521) + 1
    return torch.stack([b.sum(1), (b * w).sum(1)], 1)


def record_outputs(dev):
    """Everything the fixture holds, computed with the library that is loaded: {name: numpy array}."""
    from mvip_nerf_amd import ops, run, _lib
    from mvip_nerf_amd._lib import ptr, stream, call
    out = {}
    tr, te, _, _, _ = run.create_nerf(make_args(), device=dev)
    for net, seed in ((tr['network_fn'], 61), (tr['network_fine'], 62)):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
    ps = [p.detach() for p in (dict(tr['network_fine'].named_parameters())[k] for k in ops.PARAM_ORDER)]
    packed = ops.mlp_pack(ps)
    img = ops.mlp_pack16(ps, packed)
    w16 = ops.mlp_pack_f16x3_w16(ps, packed)
    rs = np.random.RandomState(5)
    pts = T(rs.uniform(-3., 3., size=(P_POINTS, 3)).astype(np.float32), dev)
    d = rs.standard_normal(size=(P_POINTS, 3))
    dirs = T((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32), dev)
    with torch.no_grad():
        out['points_fold'] = N(ops.mlp_points(pts, dirs, packed, ps, packed16=img))
        out['points_plain'] = N(ops.mlp_points(pts, dirs, packed, ps, packed16=ops.plain16(img)))
        out['points_f16x3_w16'] = N(ops.mlp_points(pts, dirs, packed, ps, f16x3_w16=w16))
        # rays form: S = 7 puts ray boundaries inside every wave; B S is no multiple of 128 for S = 7 and 64
        for S, B in ((7, 585), (64, 65), (128, 33)):
            rows = T(bench_like_rays(B, seed=S), dev)
            z = ops.stratified_z(rows, S, True)
            out[f'rays{S}_fold'] = N(ops.mlp_rays(rows, z, packed, ps, packed16=img))
            if S != 128:
                out[f'rays{S}_plain'] = N(ops.mlp_rays(rows, z, packed, ps, packed16=ops.plain16(img)))
            if S == 64:
                out[f'rays{S}_f16x3_w16'] = N(ops.mlp_rays(rows, z, packed, ps, f16x3_w16=w16))
            if S != 128:
                # the stash-writing training forward through the C boundary, into a zeroed stash
                n = int(_lib.load().mvip_mlp_stash_floats(B * S))
                stash = torch.zeros(n, device=dev)
                raw = torch.empty(B, S, 4, device=dev)
                call('mvip_mlp_forward_rays_stash16', ptr(ops.plain16(img)), ptr(rows), ptr(z), B, S, ptr(raw), ptr(stash),
                     stream())
                out[f'rays{S}_stash_raw'] = N(raw)
                out[f'rays{S}_stash_sums'] = N(stash_sums(stash, B * S))
                if S == 7:                 # ... and the split-precision one (fp32 tiles and ReLU sign masks)
                    stash.zero_()
                    call('mvip_mlp_forward_rays_stash_f16x3_w16', ptr(w16), ptr(rows), ptr(z), B, S, ptr(raw), ptr(stash),
                         stream())
                    out[f'rays{S}_stash_f16x3_w16_raw'] = N(raw)
                    out[f'rays{S}_stash_f16x3_w16_sums'] = N(stash_sums(stash, B * S))
                del stash
        rays = T(bench_like_rays(96, seed=96), dev)
        r = run.render_rays(rays, te['network_fn'], te['network_query_fn'], 64, lindisp=True, perturb=0., raw_noise_std=0.,
                            white_bkgd=True, N_importance=64, network_fine=te['network_fine'], retraw=True)
    for k in ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'weights', 'z_vals', 'rgb0', 'disp0', 'acc0', 'z_std'):
        out['render_' + k] = N(r[k])
    torch.cuda.synchronize()
    return out


def test_network_outputs_equal_parent_bitwise(cuda):
    """raw of the folded, unfolded, stash-writing and split-precision 16-point kernels (points form; rays form with S = 7,
    64, 128), the stash they write, and the outputs of a two-launch render of 96 rays: the bits recorded on the parent."""
    want = np.load(GOLDEN)
    got = record_outputs(cuda)
    assert set(got) == set(want.files)
    bad = []
    for k in sorted(got):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        ai = a.view(np.int32) if a.dtype == np.float32 else a
        bi = b.view(np.int32) if b.dtype == np.float32 else b
        n = int((ai != bi).sum())
        print(k, a.shape, 'differing words:', n)
        if n:
            bad.append((k, n))
    assert not bad, bad
