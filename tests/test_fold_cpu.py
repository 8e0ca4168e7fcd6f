"""feature_linear folded into the view layer (NeRF.fold_feature_inference, csrc/mlp_fwd16_fold.hip): the algebra and its
rounding on the CPU, and the numpy restatement of the folded tail of the extended weight image that tests/test_fold.py
compares the device pack against.

feature_linear has no activation, so with W' = Wv[:, :256] Wf and b' = Wv[:, :256] bf + bv

    relu(Wv cat[Wf h + bf, e_dir] + bv) = relu(W' h + Wv[:, 256:] e_dir + b').

W' and b' are accumulated in fp64 (k ascending) and rounded once to fp32, as the device pack does.  The score is
max |delta| / (2e-6 + 2e-5 |ref|): 1.0 is the tolerance tests/test_hip_kernels.py applies to the two-wave kernel.  The
bound asserted here, 0.25, is a quarter of that tolerance (measured: <= 0.07): a wrong bias term or a transposed product
gives scores in the thousands, and cannot hide inside the GPU test's tolerance."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as O
from oracle.weights import seeded_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# csrc/mlp_layout.h
PACKED_FLOATS = 597248
SEC_A_FLOATS = 593920
SEC_B_FLOATS = 3328
SB_BFOLD = 3080
FOLD_BLOCKS = 144
FOLD_TAIL_A = PACKED_FLOATS
FOLD_TAIL_B = FOLD_TAIL_A + FOLD_BLOCKS * 256
PACKED_FOLD_FLOATS = FOLD_TAIL_B + SEC_B_FLOATS


def fold_weights(sd):
    """(W' [128, 256], b' [128]) as fp32 numpy: fp64 accumulation over k = 0..255 in ascending order, one rounding.  Each
    product of two fp32 values is exact in fp64, so this is bit for bit what the device pack computes."""
    wv = np.asarray(sd['views_linears.0.weight'], np.float32).astype(np.float64)
    wf = np.asarray(sd['feature_linear.weight'], np.float32).astype(np.float64)
    bf = np.asarray(sd['feature_linear.bias'], np.float32).astype(np.float64)
    bv = np.asarray(sd['views_linears.0.bias'], np.float32).astype(np.float64)
    w = np.zeros((128, 256), np.float64)
    b = np.zeros((128,), np.float64)
    for k in range(256):
        w += wv[:, k:k + 1] * wf[k:k + 1, :]
        b += wv[:, k] * bf[k]
    return w.astype(np.float32), (b + bv).astype(np.float32)


def fold_tail_numpy(sd, section_b):
    """The tail of the extended image (floats FOLD_TAIL_A .. PACKED_FOLD_FLOATS): 144 blocks of the folded view layer
    W'' = [W' | Wv[:, 256:283] | 0] (128 x 288) in the 16-point block order -- block (to, ti), to = 0..7 output tiles of 16,
    ti = 0..17 input tiles of 16, at to * 18 + ti; float lane * 4 + s of a block, lane = (g << 4) | m, is
    W''[16 to + m][16 ti + 4 g + s] -- then `section_b` (the plain image's small vectors) with b' at SB_BFOLD."""
    w, b = fold_weights(sd)
    wv = np.asarray(sd['views_linears.0.weight'], np.float32)
    w2 = np.zeros((128, 288), np.float32)
    w2[:, :256] = w
    w2[:, 256:283] = wv[:, 256:]
    # [to, m, ti, g, s] -> [to, ti, g, m, s]
    blocks = w2.reshape(8, 16, 18, 4, 4).transpose(0, 2, 3, 1, 4)
    sb = np.array(section_b, np.float32, copy=True)
    assert sb.shape == (SEC_B_FLOATS,)
    sb[SB_BFOLD:SB_BFOLD + 128] = b
    return np.concatenate([np.ascontiguousarray(blocks).reshape(-1), sb])


def mlp_forward_folded(p, emb, w_fold, b_fold):
    """oracle.nerf_oracle.mlp_forward with the view layer evaluated on the folded weights."""
    e_pts, e_dir = emb[:, :63], emb[:, 63:]
    h = e_pts
    for i in range(8):
        h = F.relu(F.linear(h, p[f'pts_linears.{i}.weight'], p[f'pts_linears.{i}.bias']))
        if i == 4:
            h = torch.cat([e_pts, h], -1)
    sigma = F.linear(h, p['alpha_linear.weight'], p['alpha_linear.bias'])
    wcat = torch.cat([w_fold, p['views_linears.0.weight'][:, 256:]], -1)
    v = F.relu(F.linear(torch.cat([h, e_dir], -1), wcat, b_fold))
    rgb = F.linear(v, p['rgb_linear.weight'], p['rgb_linear.bias'])
    return torch.cat([rgb, sigma], -1)


def score(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (2e-6 + 2e-5 * np.abs(ref))).max())


def seeded_points(n, seed):
    """n points of the scene box of the bench workload and unit view directions, encoded: [n, 90] fp64."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-4., 4., size=(n, 3))
    d = rs.standard_normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    pts, d = torch.from_numpy(pts.astype(np.float32)).double(), torch.from_numpy(d.astype(np.float32)).double()
    return torch.cat([O.posenc(pts, 10), O.posenc(d, 4)], -1)


def weight_set(seed, scale):
    sd = seeded_state_dict(seed)
    for k in ('feature_linear.weight', 'views_linears.0.weight'):
        sd[k] = (sd[k] * np.float32(scale)).astype(np.float32)
    return sd


def _folded_and_plain(sd, emb32):
    p32 = {k: torch.from_numpy(v) for k, v in sd.items()}
    w, b = fold_weights(sd)
    with torch.no_grad():
        return (mlp_forward_folded(p32, emb32, torch.from_numpy(w), torch.from_numpy(b)).numpy(),
                O.mlp_forward(p32, emb32).numpy())


def test_fold_against_golden_forward():
    g = dict(np.load(os.path.join(GOLDEN, 'mlp_fwd_bwd.npz'), allow_pickle=False))
    sd = seeded_state_dict(int(g['seed']))
    folded, plain = _folded_and_plain(sd, torch.from_numpy(g['emb']))
    s_fold, s_plain = score(folded, g['out']), score(plain, g['out'])
    print(f'golden: unfolded {s_plain:.4f}  folded {s_fold:.4f}')
    assert s_fold <= 0.25
    np.testing.assert_array_equal(folded[:, 3], plain[:, 3])          # sigma does not pass through the fold


@pytest.mark.parametrize('seed,scale', [(77, 1.0), (0, 1.0), (1, 3.0)])
def test_fold_against_fp64_network(seed, scale):
    sd = weight_set(seed, scale)
    emb64 = seeded_points(20000, seed + 1000)
    with torch.no_grad():
        ref = O.mlp_forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, emb64).numpy()
    folded, plain = _folded_and_plain(sd, emb64.float())
    s_fold, s_plain = score(folded, ref), score(plain, ref)
    print(f'seed {seed} scale {scale}: unfolded {s_plain:.4f}  folded {s_fold:.4f}')
    assert s_fold <= 0.25
    # the fold removes a rounding stage: it must not be further from the fp64 network than the unfolded fp32 network by
    # more than that network's own distance
    assert s_fold <= 2 * s_plain + 0.01


def test_fold_detects_wrong_algebra():
    """The bound is tight enough to catch what it is there for: b' without the Wv bf term, and W' from the transposed Wf."""
    sd = seeded_state_dict(77)
    emb64 = seeded_points(2000, 5)
    p32 = {k: torch.from_numpy(v) for k, v in sd.items()}
    w, b = fold_weights(sd)
    with torch.no_grad():
        ref = O.mlp_forward({k: v.double() for k, v in p32.items()}, emb64).numpy()
        no_bf = mlp_forward_folded(p32, emb64.float(), torch.from_numpy(w), p32['views_linears.0.bias']).numpy()
        wt = (sd['views_linears.0.weight'][:, :256].astype(np.float64) @ sd['feature_linear.weight'].astype(np.float64).T)
        transposed = mlp_forward_folded(p32, emb64.float(), torch.from_numpy(wt.astype(np.float32)), torch.from_numpy(b)).numpy()
    assert score(no_bf, ref) > 10 and score(transposed, ref) > 10


def test_fold_tail_layout():
    """Block order of the tail: spot values against the definition, sizes against csrc/mlp_layout.h."""
    sd = seeded_state_dict(3)
    sb = np.arange(SEC_B_FLOATS, dtype=np.float32)
    tail = fold_tail_numpy(sd, sb)
    assert tail.size == PACKED_FOLD_FLOATS - PACKED_FLOATS == 144 * 256 + SEC_B_FLOATS
    assert SEC_A_FLOATS + SEC_B_FLOATS == PACKED_FLOATS and SB_BFOLD + 128 <= SEC_B_FLOATS
    w, b = fold_weights(sd)
    wv = sd['views_linears.0.weight']
    for to, ti, m, g_, s in ((0, 0, 0, 0, 0), (3, 5, 7, 2, 1), (7, 15, 15, 3, 3), (2, 16, 4, 1, 2), (7, 17, 15, 2, 2), (5, 17, 0, 2, 3)):
        row, col = 16 * to + m, 16 * ti + 4 * g_ + s
        want = w[row, col] if col < 256 else (wv[row, col] if col < 283 else 0.)
        assert tail[(to * 18 + ti) * 256 + ((g_ << 4) | m) * 4 + s] == want, (to, ti, m, g_, s)
    secb = tail[144 * 256:]
    np.testing.assert_array_equal(secb[SB_BFOLD:SB_BFOLD + 128], b)
    np.testing.assert_array_equal(secb[:SB_BFOLD], sb[:SB_BFOLD])
    np.testing.assert_array_equal(secb[SB_BFOLD + 128:], sb[SB_BFOLD + 128:])
    # fp64 reference of the product: the sequential sum rounds to within 1 ulp of the exactly rounded matrix product
    exact = (wv[:, :256].astype(np.float64) @ sd['feature_linear.weight'].astype(np.float64)).astype(np.float32)
    assert np.abs(w - exact).max() <= np.spacing(np.abs(exact).max())
