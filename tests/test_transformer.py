"""The SD UNet's transformer-block kernels (csrc/attention.hip, csrc/transformer.hip, guidance/transformer_cm.py)
against the fp64 statement of the same expressions on the host.  Tolerances are fractions of the output scale:
split-precision MFMA products (fp16 hi+lo operands, three products, fp32 accumulation) are fp32-grade, ~1e-6."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def N(t):
    return t.detach().cpu().numpy()


def _attention_case(cuda, Nb, heads, D, Lq, Lk, LqP=None, seed=0, q_gain=1.0, flags=0):
    """q, k, v channel-major [Nb, heads*D, L] fp32 -> HIP attention vs fp64 softmax(q^T k / sqrt(D)) v."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(seed)
    DP = (D + 15) // 16 * 16
    LqP = LqP or Lq
    LkP = (Lk + 63) // 64 * 64
    q = torch.randn(Nb, heads, D, Lq, generator=gen) * q_gain
    k = torch.randn(Nb, heads, D, Lk, generator=gen) * 1.3
    v = torch.randn(Nb, heads, D, Lk, generator=gen) * 0.7 + 0.1
    s = torch.einsum('nhdi,nhdj->nhij', q.double(), k.double()) * D ** -0.5
    ref = torch.einsum('nhij,nhdj->nhdi', torch.softmax(s, -1), v.double()).reshape(Nb, heads * D, Lq)

    def padded(t, L, LP):                      # [Nb, heads*DP, LP] with zero channels D..DP-1 and zero tokens >= L
        out = torch.zeros(Nb, heads, DP, LP)
        out[:, :, :D, :L] = t
        return out.reshape(Nb, heads * DP, LP).to(cuda)
    R = heads * DP
    qd, kd, vd = padded(q, Lq, LqP), padded(k, Lk, LkP), padded(v, Lk, LkP)
    sq, sk, sv = (ops.absmax_scale(t) for t in (qd, kd, vd))
    qs = ops.split_planes_strided(qd, Nb, R, Lq, R * LqP, LqP, 1, sq)
    ks = ops.split_planes_strided(kd, Nb, R, LkP, R * LkP, LkP, 1, sk)
    vp = ops.attention_pack_v(vd, Nb, heads, D, DP, Lk, LkP, R * LkP, LkP, 1, sv)
    old = ops.ATTENTION_FLAGS
    ops.ATTENTION_FLAGS = flags
    try:
        out = ops.attention_f16x3(qs, ks, vp, sq, sk, sv, Nb, heads, D, Lq, LqP, Lk, LkP)
    finally:
        ops.ATTENTION_FLAGS = old
    assert out.shape == (Nb, heads * D, LqP)
    got = N(out)[:, :, :Lq]
    scale = float(ref.abs().max())
    err = np.abs(got - ref.numpy()).max() / scale
    return err, got, ref.numpy()


@pytest.mark.parametrize('heads,D,Lq,Lk,LqP,flags', [
    (8, 40, 256, 256, None, 0), (8, 40, 256, 256, None, 1), (2, 40, 1024, 1024, None, 0),   # 64x64-level heads
    (8, 80, 256, 256, None, 0), (3, 80, 128, 1024, None, 0),                                 # 32x32 level
    (8, 160, 256, 256, None, 0), (8, 160, 64, 64, 256, 0),                                   # 16x16 and (padded) 8x8
    (8, 40, 256, 77, None, 0), (8, 40, 128, 77, None, 1), (8, 80, 64, 77, None, 0), (8, 160, 64, 77, 256, 0),  # prompt
    (1, 40, 32, 1, None, 0), (1, 80, 96, 33, None, 0)])                                      # ragged key counts
def test_attention_vs_fp64(cuda, heads, D, Lq, Lk, LqP, flags):
    err, got, ref = _attention_case(cuda, 2, heads, D, Lq, Lk, LqP, seed=heads + D + Lq + Lk, flags=flags)
    assert err < 3e-6, err


def test_attention_peaked_and_uniform_scores(cuda):
    """Peaked softmax (large logits: one key dominates) and exactly uniform scores (q = 0: every probability is
    1/Lk, the case where the fp16 lo terms of the probabilities matter most)."""
    err, _, _ = _attention_case(cuda, 1, 8, 40, 256, 4096, seed=5, q_gain=6.0)
    assert err < 3e-6, err
    err, got, ref = _attention_case(cuda, 1, 8, 40, 128, 4096, seed=6, q_gain=0.0)
    assert err < 2e-6, err
    err, _, _ = _attention_case(cuda, 1, 8, 80, 128, 1024, seed=7, q_gain=0.0)
    assert err < 2e-6, err


def test_attention_full_size_level(cuda):
    """The UNet's largest attention (2 x 8 heads x 4096 x 4096 x 40) on a strided sample of rows vs fp64."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(11)
    Nb, heads, D, L = 2, 8, 40, 4096
    DP, R = 48, 8 * 48
    q = torch.randn(Nb, heads, D, L, generator=gen)
    k = torch.randn(Nb, heads, D, L, generator=gen)
    v = torch.randn(Nb, heads, D, L, generator=gen)

    def padded(t):
        out = torch.zeros(Nb, heads, DP, L)
        out[:, :, :D] = t
        return out.reshape(Nb, R, L).to(cuda)
    qd, kd, vd = padded(q), padded(k), padded(v)
    sq, sk, sv = (ops.absmax_scale(t) for t in (qd, kd, vd))
    qs = ops.split_planes_strided(qd, Nb, R, L, R * L, L, 1, sq)
    ks = ops.split_planes_strided(kd, Nb, R, L, R * L, L, 1, sk)
    vp = ops.attention_pack_v(vd, Nb, heads, D, DP, L, L, R * L, L, 1, sv)
    out = ops.attention_f16x3(qs, ks, vp, sq, sk, sv, Nb, heads, D, L, L, L, L)      # 256-query workgroups (8 waves)
    ops.ATTENTION_FLAGS = 2
    try:
        narrow = ops.attention_f16x3(qs, ks, vp, sq, sk, sv, Nb, heads, D, L, L, L, L)   # 128-query workgroups
    finally:
        ops.ATTENTION_FLAGS = 0
    assert torch.equal(out, narrow)              # the workgroup shape changes no arithmetic
    rows = torch.arange(0, L, 37)
    s = torch.einsum('nhdi,nhdj->nhij', q[..., rows].double(), k.double()) * D ** -0.5
    ref = torch.einsum('nhij,nhdj->nhdi', torch.softmax(s, -1), v.double()).reshape(Nb, heads * D, -1)
    got = N(out)[:, :, rows.numpy()]
    assert np.abs(got - ref.numpy()).max() / float(ref.abs().max()) < 3e-6


def test_layernorm_split_feeds_gemm(cuda):
    """LayerNorm over the (strided) channel axis written as split planes, consumed by the GEMM: W LN(x) vs fp64;
    the padded-token variant (L = 64 inside LP = 256) leaves zero columns."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(3)
    for Nb, C, L, LP, M in ((2, 320, 256, 256, 64), (2, 1280, 64, 256, 96), (1, 640, 1024, 1024, 32)):
        x = torch.randn(Nb, C, LP, generator=gen) * 2.0 + 0.5
        g = torch.randn(C, generator=gen) * 0.3 + 1.0
        b = torch.randn(C, generator=gen) * 0.2
        W = torch.randn(M, C, generator=gen) / C ** 0.5
        ln = torch.nn.functional.layer_norm(x.double().transpose(1, 2), (C,), g.double(), b.double(), 1e-5)   # [Nb, LP, C]
        ref = torch.einsum('mc,nlc->nml', W.double(), ln)
        ref[:, :, L:] = 0
        xs = ops.layernorm_split(x.to(cuda), g.to(cuda), b.to(cuda), 1e-5, Nb, C, L, LP, 16.0)
        s2 = torch.tensor([16.0, 1 / 16.0, 0, 0], device=cuda)
        y = ops.gemm_f16x3(xs, ops.gemm_pack_a(W.to(cuda), M, C, C, 1), Nb, C, M, LP, x_scale2=s2)
        np.testing.assert_allclose(N(y), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()))


def test_layernorm_statistics_from_the_producing_gemm(cuda):
    """Round 6 (VERDICT r5 task 2): a projection that writes the residual stream leaves the NEXT LayerNorm's statistics from its
    epilogue (mvip_gemm_f16x3_ws_ln: per token and 32 / 64-row segment the fp64 sum and sum of squares of the finished rows, bias
    and residual included), and mvip_layernorm_split_planes_stats normalises from them: one launch instead of two, no pass over
    the tensor for its moments.  Checked per shape of the UNet's levels: y is bit-equal to the plain GEMM's, the partial moments
    equal fp64 sums of y's rows, the planes equal those of the two-launch LayerNorm (the same fp64 statistics up to the order
    of the additions: bit-equal in all but a handful of elements) and W2 LN(y) agrees with fp64.  A split-K shape declines
    (segments = 0) and falls back."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(8)
    lib = ops._lib.load()
    for Nb, C, L, LP in ((2, 320, 4096, 4096), (2, 640, 1024, 1024), (1, 320, 256, 256), (2, 1280, 64, 256)):
        K = C
        x = torch.randn(Nb, K, LP, generator=gen)
        W = torch.randn(C, K, generator=gen) / K ** 0.5
        bias = torch.randn(C, generator=gen) * 0.1
        res = torch.randn(Nb, C, LP, generator=gen) * 3.0 + 1.5              # a residual stream with a mean (cancellation in E[x^2] - mean^2)
        g = torch.randn(C, generator=gen) * 0.3 + 1.0
        b = torch.randn(C, generator=gen) * 0.2
        xd, s2 = ops._scaled_planes(x.to(cuda), Nb, K, LP, K * LP, LP, 1)
        packed = ops.gemm_pack_a(W.to(cuda), C, K, K, 1, weights=True)
        S = int(lib.mvip_gemm_ln_segments(Nb, K, C, LP, ops._prec_w(packed)))
        y0 = ops.gemm_f16x3(xd, packed, Nb, K, C, LP, bias=bias.to(cuda), residual=res.to(cuda), x_scale2=s2)
        y1, st = ops.gemm_f16x3(xd, packed, Nb, K, C, LP, bias=bias.to(cuda), residual=res.to(cuda), x_scale2=s2, ln_stats=True)
        assert torch.equal(y0, y1)
        if C == 1280:                                                       # 80 workgroups x 40 stages: split over K
            assert S == 0 and st is None
            continue
        assert S in (C // 32, C // 64) and st is not None and st[1] == S
        part = st[0].reshape(Nb, S, 2, LP).cpu().numpy()
        yd = y1.double().cpu().reshape(Nb, S, C // S, LP)
        np.testing.assert_allclose(part[:, :, 0], yd.sum(2).numpy(), rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(part[:, :, 1], (yd * yd).sum(2).numpy(), rtol=1e-12)
        a = ops.layernorm_split(y1, g.to(cuda), b.to(cuda), 1e-5, Nb, C, L, LP, 16.0)
        c = ops.layernorm_split(y1, g.to(cuda), b.to(cuda), 1e-5, Nb, C, L, LP, 16.0, stats=st)
        same = float((a == c).float().mean())
        assert same > 0.999, same
        af, cf = a.float().cpu().numpy(), c.float().cpu().numpy()
        assert np.abs(af - cf).max() <= 2e-3 * max(np.abs(af).max(), 1.0)   # a differing hi half moves by one fp16 ulp at most
        M2 = 64
        W2 = torch.randn(M2, C, generator=gen) / C ** 0.5
        sc = torch.tensor([16.0, 1 / 16.0, 0, 0], device=cuda)
        out = ops.gemm_f16x3(c, ops.gemm_pack_a(W2.to(cuda), M2, C, C, 1), Nb, C, M2, LP, x_scale2=sc)
        ln = torch.nn.functional.layer_norm(y1.double().cpu().transpose(1, 2), (C,), g.double(), b.double(), 1e-5)
        ref = torch.einsum('mc,nlc->nml', W2.double(), ln)
        ref[:, :, L:] = 0
        np.testing.assert_allclose(N(out), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()))


def test_geglu_and_linear_small(cuda):
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(4)
    Nb, R, L, LP = 2, 96, 200, 256
    y = torch.randn(Nb, 2 * R, LP, generator=gen) * 2.0
    ref = y[:, :R].double() * torch.nn.functional.gelu(y[:, R:].double())
    ref[:, :, L:] = 0
    out, s2 = ops.geglu(y.to(cuda), Nb, R, L, LP)
    np.testing.assert_allclose(N(out), ref.float().numpy(), rtol=2e-6, atol=2e-6)
    s = float(s2[0])
    assert 512.0 <= float(ref.abs().max()) * s < 1024.0 and abs(float(s2[1]) * s - 1.0) < 1e-7
    for NB, M, K, act in ((2, 1280, 320, 0), (2, 321, 1280, 1), (8, 7, 50, 1), (1, 64, 64, 0)):
        x = torch.randn(NB, K, generator=gen)
        W = torch.randn(M, K, generator=gen) / K ** 0.5
        b = torch.randn(M, generator=gen)
        xin = torch.nn.functional.silu(x.double()) if act else x.double()
        ref = xin @ W.double().t() + b.double()
        got = ops.linear_small(x.to(cuda), W.to(cuda), b.to(cuda), act_in=act)
        np.testing.assert_allclose(N(got), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()))


def test_absmax_scale_sections(cuda):
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(3, 4, 1001, generator=gen)
    x[:, 1] *= 100.0
    x[:, 2] *= 1e-3
    x[1, 3, 5] = float('nan')
    sc = N(ops.absmax_scale_sections(x.to(cuda), 3, 4, 1001)).reshape(4, 4)
    for s in range(4):
        m = float(torch.nan_to_num(x[:, s], nan=0.0).abs().max())
        assert 512.0 <= m * sc[s, 0] < 1024.0 and sc[s, 0] * sc[s, 1] == 1.0


def _scale_rule(x):
    """The scale rule of csrc/f16x3_operand.h restated in numpy: {s, 1/s} as fp32 for the tensor x."""
    a = np.abs(np.asarray(x, dtype=np.float32).ravel())
    a = a[~np.isnan(a) & (a < np.float32(3.0e38))]
    m = np.float32(a.max()) if a.size else np.float32(0.0)
    s = np.float32(1.0) if m == 0 else np.float32(2.0 ** int(np.clip(10 - np.frexp(np.float32(m))[1], -60, 60)))
    return np.array([s, np.float32(1.0) / s], dtype=np.float32)


def test_scale_rule_every_producer(cuda):
    """Every producer of a power-of-two scale against the numpy restatement of the ONE rule, both words bit for bit."""
    from mvip_nerf_amd import ops

    def same(got, x, what):
        got, want = np.ascontiguousarray(np.asarray(got.cpu() if torch.is_tensor(got) else got).ravel()[:2]), _scale_rule(x)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (what, got.tolist(), want.tolist())
        return want

    gen = torch.Generator().manual_seed(31)
    # ops.absmax_scale, one launch and three: 49,157 floats = four workgroups, a trip of the 8-deep loop, the single-vector
    # loop and the scalar tail; the same sliced [1:] (unaligned: the scalar path); 100 floats (one workgroup)
    maxima = (0.0, 512.0, 1023.5, 0.3, 1e-30, 1e30)
    expect = {0.0: 1.0, 512.0: 1.0, 1e-30: 2.0 ** 60, 1e30: 2.0 ** -60}
    base = {49157: torch.rand(49157, generator=gen) * 1.8 - 0.9, 100: torch.rand(100, generator=gen) * 1.8 - 0.9}
    old = ops.ABSMAX_THREE_LAUNCHES
    try:
        for three in (False, True):
            ops.ABSMAX_THREE_LAUNCHES = three
            for n, unit in base.items():
                for i, mx in enumerate(maxima):
                    for junk in (False, True):
                        x = unit * mx                                    # |x| <= 0.9 mx, then the maximum itself
                        x[(5, 4 * 9000 + 1, n - 1)[i % 3] % n] = -mx if i & 1 else mx    # 8-deep loop / vector loop / tail
                        if junk:
                            x[3], x[n // 2], x[n - 2] = float('nan'), float('inf'), 3.2e38
                        xd = x.to(cuda)
                        for off in ((0, 1) if n > 100 else (0,)):        # sliced on the device: a pointer 4 bytes off
                            want = same(ops.absmax_scale(xd[off:]), x[off:], ('absmax_scale', three, n, mx, junk, off))
                            if mx in expect:
                                assert want[0] == np.float32(expect[mx])
    finally:
        ops.ABSMAX_THREE_LAUNCHES = old

    # ops.absmax_scale_sections: an exact power of two in section 0, NaN / inf / 3.2e38 planted in sections 3, 2, 1
    x = torch.randn(3, 4, 1001, generator=gen).clamp_(-4.0, 4.0)
    x[:, 1] *= 100.0
    x[:, 2] *= 1e-3
    x[2, 0, 7] = -1024.0
    x[1, 3, 5], x[0, 2, 1000], x[2, 1, 0] = float('nan'), float('inf'), 3.2e38
    sc = N(ops.absmax_scale_sections(x.to(cuda), 3, 4, 1001)).reshape(4, 4)
    for s in range(4):
        want = same(sc[s], x[:, s], ('sections', s))
    assert _scale_rule(x[:, 0])[0] == np.float32(0.5)

    # ops.geglu: the rule on the tensor it returns.  value 64, gate 8: gelu(8) = 8 in fp32, the product is 512 exactly
    Nb, R, L, LP = 2, 96, 200, 256
    y = torch.randn(Nb, 2 * R, LP, generator=gen) * 2.0
    for case in ('pow2', 'nan'):
        yc = y.clone()
        if case == 'pow2':
            yc[1, 17, 33], yc[1, R + 17, 33] = 64.0, 8.0
        else:
            yc[0, 5, 9] = float('nan')
        out, s2 = ops.geglu(yc.to(cuda), Nb, R, L, LP)
        want = same(s2, N(out), ('geglu', case))
        if case == 'pow2':
            assert float(N(out)[1, 17, 33]) == 512.0 and want[0] == np.float32(1.0)
        else:
            assert np.isnan(N(out)[0, 5, 9])

    # ops.gemm_geglu_f16x3 (the GEMM's epilogue collects the maximum): zero weight rows with bias 64 / 8 -> 512 exactly;
    # a NaN bias -> one NaN row
    K, P = 32, 256
    xg = torch.randn(Nb, K, P, generator=gen)
    s2x = ops.absmax_scale(xg.to(cuda))
    xs = ops.split_planes_strided(xg.to(cuda), Nb, K, P, K * P, P, 1, s2x)
    W = torch.randn(2 * R, K, generator=gen) / K ** 0.5
    b = torch.randn(2 * R, generator=gen) * 0.2
    for case in ('pow2', 'nan'):
        Wc, bc = W.clone(), b.clone()
        if case == 'pow2':
            Wc[17], Wc[R + 17] = 0.0, 0.0
            bc[17], bc[R + 17] = 64.0, 8.0
        else:
            bc[5] = float('nan')
        wi, bi = ops.geglu_interleave(Wc.to(cuda), bc.to(cuda))
        out, s2 = ops.gemm_geglu_f16x3(xs, ops.gemm_pack_a(wi, 2 * R, K, K, 1), bi, Nb, K, 2 * R, P, L, x_scale2=s2x)
        want = same(s2, N(out), ('gemm_geglu', case))
        if case == 'pow2':
            assert float(N(out)[1, 17, 33]) == 512.0 and want[0] == np.float32(1.0)
        else:
            assert np.isnan(N(out)[0, 5, :L]).all()

    # the {scale, 1/scale} words at the start of the packed images' 256-byte tails
    for case in ('pow2', 'nan'):
        w = torch.randn(32, 16, 3, 3, generator=gen).clamp_(-3.0, 3.0) * 0.05
        a = torch.randn(32, 32, generator=gen).clamp_(-3.0, 3.0) * 0.05
        if case == 'pow2':
            w[7, 3, 1, 2], a[9, 30] = 0.25, -0.25
        else:
            w[7, 3, 1, 2], a[9, 30] = float('nan'), float('nan')
        pk = ops.conv3x3_pack(w.to(cuda))
        want = same(pk[32 * 16 * 36:32 * 16 * 36 + 8].view(torch.float32), w, ('conv3x3_pack', case))
        pa = ops.gemm_pack_a(a.to(cuda), 32, 32, 32, 1)
        want_a = same(pa[32 * 32 * 4:32 * 32 * 4 + 8].view(torch.float32), a, ('gemm_pack_a', case))
        if case == 'pow2':
            assert want[0] == np.float32(2048.0) and want_a[0] == np.float32(2048.0)


# ---- contractions that hand each other operands (csrc/plane_sink.h) --------------------------------------------------
def decode_planes(buf, Nb, rows, P):
    """fp16 hi/lo split planes [Nb][rows/16][kg 2][hl 2][P][8] -> float64 [Nb, rows, P] (hi + lo)."""
    t = buf.view(Nb, rows // 16, 2, 2, P, 8).double().cpu()
    v = t[:, :, :, 0] + t[:, :, :, 1]                          # [Nb, ck, kg, P, 8]
    return v.permute(0, 1, 2, 4, 3).reshape(Nb, rows, P)


def decode_vfrag(buf, Nb, blocks, P):
    """attention V fragments [Nb][blocks][P/16][hl 2][lane 64][8 halves] -> float64 [Nb, blocks*32 rows, P keys]:
    element j of lane (l32, hh) of 16-key group s is row l32, key 16 s + 8 (j >> 2) + 4 hh + (j & 3)."""
    t = buf.view(torch.float16).view(Nb, blocks, P // 16, 2, 2, 32, 8).double().cpu()     # [.., s16, hl, hh, l32, j]
    v = t[:, :, :, 0] + t[:, :, :, 1]                                                      # [Nb, blk, s16, hh, l32, j]
    out = torch.zeros(Nb, blocks, 32, P, dtype=torch.float64)
    for hh in range(2):
        for j in range(8):
            keys = torch.arange(P // 16) * 16 + 8 * (j >> 2) + 4 * hh + (j & 3)
            out[:, :, :, keys] = v[:, :, :, hh, :, j].permute(0, 1, 3, 2)
    return out.reshape(Nb, blocks * 32, P)


@pytest.mark.parametrize('Nb,K,P,rq,rv,v_dt', [(2, 320, 256, 384, 512, 2), (1, 640, 512, 640, 768, 3), (2, 1280, 256, 1280, 1280, 5),
                                                (1, 64, 256, 64, 0, 1)])
def test_gemm_sinks_vs_fp64(cuda, Nb, K, P, rq, rv, v_dt):
    """mvip_gemm_f16x3_sinks: one GEMM whose row sections leave as Q planes, K planes and (transposed launch) attention
    V fragments at three different fixed power-of-two scales, against W X + b in fp64 -- decoded from the operand
    formats themselves (hi + lo), so layout, exchange and scales are all checked.  5e-6 of each section's scale."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(K + P)
    M = 2 * rq + rv
    x = torch.randn(Nb, K, P, generator=gen) * 1.7
    W = torch.randn(M, K, generator=gen) / K ** 0.5
    b = torch.randn(M, generator=gen) * 0.3
    ref = torch.einsum('mk,nkp->nmp', W.double(), x.double()) + b.double()[None, :, None]
    s2 = ops.absmax_scale(x.to(cuda))
    xs = ops.split_planes_strided(x.to(cuda), Nb, K, P, K * P, P, 1, s2)
    secs = [(rq, 'planes', 0.5), (rq, 'planes', 64.0)] + ([(rv, 'vfrag', 4.0)] if rv else [])
    bufs = ops.gemm_f16x3_sinks(xs, ops.gemm_pack_a(W.to(cuda), M, K, K, 1), Nb, K, P, secs, bias=b.to(cuda), x_scale2=s2,
                                v_dt=v_dt)
    torch.cuda.synchronize()
    row = 0
    for (rows, kind, sc), buf in zip(secs, bufs):
        want = ref[:, row:row + rows] * sc
        got = decode_planes(buf, Nb, rows, P) if kind == 'planes' else decode_vfrag(buf, Nb, rows // 32, P)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=5e-6 * float(want.abs().max()), err_msg=f'{kind}@{row}')
        row += rows


def test_gemm_geglu_sink_vs_fp64(cuda):
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(21)
    Nb, K, R, P, L = 2, 320, 256, 512, 450
    x = torch.randn(Nb, K, P, generator=gen)
    W = torch.randn(2 * R, K, generator=gen) / K ** 0.5
    b = torch.randn(2 * R, generator=gen) * 0.2
    y = torch.einsum('mk,nkp->nmp', W.double(), x.double()) + b.double()[None, :, None]
    ref = y[:, :R] * torch.nn.functional.gelu(y[:, R:])
    ref[:, :, L:] = 0
    wi, bi = ops.geglu_interleave(W.to(cuda), b.to(cuda))
    s2 = ops.absmax_scale(x.to(cuda))
    xs = ops.split_planes_strided(x.to(cuda), Nb, K, P, K * P, P, 1, s2)
    out = ops.gemm_geglu_f16x3_sink(xs, ops.gemm_pack_a(wi, 2 * R, K, K, 1), bi, Nb, K, 2 * R, P, L, 8.0, x_scale2=s2)
    got = decode_planes(out, Nb, R, P) / 8.0
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=5e-6 * float(ref.abs().max()))
    assert float(got[:, :, L:].abs().max()) == 0.0


@pytest.mark.parametrize('Nb,K,M,P', [(2, 1280, 320, 512), (2, 5120, 1280, 256), (1, 2560, 640, 1024)])
def test_gemm_planes_with_residual_and_split_k_vs_fp64(cuda, Nb, K, M, P):
    """(W X + b + residual) * scale as operand planes, incl. the shapes whose grid is split over K (partial sums + the
    reduce-to-planes launch): decoded planes vs fp64, and the planes feed a second GEMM."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(K + M)
    x = torch.randn(Nb, K, P, generator=gen)
    W = torch.randn(M, K, generator=gen) / K ** 0.5
    b = torch.randn(M, generator=gen) * 0.2
    res = torch.randn(Nb, M, P, generator=gen) * 3.0
    ref = torch.einsum('mk,nkp->nmp', W.double(), x.double()) + b.double()[None, :, None] + res.double()
    s2 = ops.absmax_scale(x.to(cuda))
    xs = ops.split_planes_strided(x.to(cuda), Nb, K, P, K * P, P, 1, s2)
    planes = ops.gemm_f16x3_planes(xs, ops.gemm_pack_a(W.to(cuda), M, K, K, 1), Nb, K, M, P, 16.0, bias=b.to(cuda),
                                   residual=res.to(cuda), x_scale2=s2)
    got = decode_planes(planes, Nb, M, P) / 16.0
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=5e-6 * float(ref.abs().max()))
    W2 = torch.randn(64, M, generator=gen) / M ** 0.5
    y = ops.gemm_f16x3(planes, ops.gemm_pack_a(W2.to(cuda), 64, M, M, 1), Nb, M, 64, P, x_scale2=ops.scale2_tensor(16.0, cuda))
    ref2 = torch.einsum('mk,nkp->nmp', W2.double(), ref)
    np.testing.assert_allclose(N(y), ref2.float().numpy(), rtol=0, atol=6e-6 * float(ref2.abs().max()))


@pytest.mark.parametrize('heads,D,L,LP', [(8, 40, 256, 256), (8, 80, 256, 256), (8, 160, 64, 256), (4, 40, 1024, 1024), (8, 40, 4096, 4096)])
def test_attention_between_sinks_vs_fp64(cuda, heads, D, L, LP):
    """q / k / v projection (sinks) -> attention (operands at the GEMM's strides, result as operand planes) -> output
    projection, against the fp64 statement; fixed scales chosen 2^6 .. 2^9 too wide on purpose."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(heads * D + L)
    Nb, C = 2, heads * D
    DP, DT = (D + 15) // 16 * 16, (D + 31) // 32
    R, RV = heads * DP, heads * DT * 32
    x = torch.zeros(Nb, C, LP)
    x[:, :, :L] = torch.randn(Nb, C, L, generator=gen)
    Wq, Wk, Wv, Wo = (torch.randn(C, C, generator=gen) / C ** 0.5 * g for g in (2.0, 2.0, 1.0, 1.0))
    bo = torch.randn(C, generator=gen) * 0.1
    q, k, v = (torch.einsum('mk,nkp->nmp', Wm.double(), x.double()[:, :, :L]).reshape(Nb, heads, D, L) for Wm in (Wq, Wk, Wv))
    att = torch.softmax(torch.einsum('nhdi,nhdj->nhij', q, k) * D ** -0.5, -1)
    o = torch.einsum('nhij,nhdj->nhdi', att, v).reshape(Nb, C, L)
    ref = torch.einsum('mk,nkp->nmp', Wo.double(), o) + bo.double()[None, :, None]

    def pad_rows(Wm, rows):
        out = torch.zeros(heads * rows, C)
        out.view(heads, rows, C)[:, :D] = Wm.view(heads, D, C)
        return out
    Wqkv = torch.cat([pad_rows(Wq, DP), pad_rows(Wk, DP), pad_rows(Wv, DT * 32)], 0).to(cuda)
    xd = x.to(cuda)
    s2 = ops.absmax_scale(xd)
    xs = ops.split_planes_strided(xd, Nb, C, LP, C * LP, LP, 1, s2)
    bound = float(x.abs().max()) * max(float(Wm.abs().sum(1).max()) for Wm in (Wq, Wk, Wv))
    sq, sk, sv = (ops.pow2_scale_for_bound(bound * f) for f in (1.0, 8.0, 64.0))
    qs, ks, vp = ops.gemm_f16x3_sinks(xs, ops.gemm_pack_a(Wqkv, 2 * R + RV, C, C, 1), Nb, C, LP,
                                      [(R, 'planes', sq), (R, 'planes', sk), (RV, 'vfrag', sv)], x_scale2=s2, v_dt=DT)
    tq, tk, tv = (ops.scale2_tensor(t, cuda) for t in (sq, sk, sv))
    op = ops.attention_f16x3_sink(qs, ks, vp, tq, tk, tv, Nb, heads, D, L, LP, L, L, LP, LP, LP // 16)
    y = ops.gemm_f16x3(op, ops.gemm_pack_a(Wo.to(cuda), C, C, C, 1), Nb, C, C, LP, bias=bo.to(cuda), x_scale2=tv)
    np.testing.assert_allclose(N(y)[:, :, :L], ref.float().numpy(), rtol=0, atol=6e-6 * float(ref.abs().max()))
    assert torch.isfinite(y).all()


@pytest.mark.parametrize('sinks', [True, False])
@pytest.mark.parametrize('C,heads,H,W', [(320, 8, 16, 16), (640, 8, 16, 16), (1280, 8, 16, 16), (1280, 8, 8, 8)])
def test_transformer2d_hip_path_vs_fp64_module(cuda, C, heads, H, W, sinks):
    """Transformer2DModel (GroupNorm, proj_in, self-attention, cross-attention, GEGLU, proj_out, residual) on the
    HIP kernels vs the SAME module evaluated in fp64 by torch on the host."""
    from mvip_nerf_amd.guidance import sd_nets, transformer_cm
    torch.manual_seed(C + H)
    transformer_cm.USE_SINKS = sinks       # True: contractions hand each other operands at bound-based scales (default)
    mod = sd_nets.Transformer2DModel(C, heads, 768).eval()
    with torch.no_grad():
        for name, p in mod.named_parameters():                     # non-trivial norms and biases
            if 'norm' in name:
                p.add_(torch.randn_like(p) * 0.2)
    for p in mod.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, C, H, W) * 1.5
    ctx = torch.randn(2, 77, 768)
    with torch.no_grad():
        ref = mod.double()(x.double(), ctx.double())
    mod = mod.float().to(cuda)
    xd, cd = x.to(cuda), ctx.to(cuda)
    assert transformer_cm.supported(mod, xd)
    with torch.no_grad():
        got = mod(xd, cd)
        again = mod(xd, cd)                                        # cached prompt projections
    assert torch.equal(got, again)
    scale = float(ref.abs().max())
    np.testing.assert_allclose(N(got), ref.float().numpy(), rtol=0, atol=1e-5 * scale)
    from mvip_nerf_amd import ops
    assert ops.FORWARD_UNIT_SCALE is False                         # default: measured (magnitude-invariant) scales
    ops.FORWARD_UNIT_SCALE = True                                  # opt-in: fixed scale 1 for forward activations
    try:
        with torch.no_grad():
            unit = mod(xd, cd)
    finally:
        ops.FORWARD_UNIT_SCALE = False
    np.testing.assert_allclose(N(unit), ref.float().numpy(), rtol=0, atol=1e-5 * scale)   # O(1) activations: same grade
    # a changed weight invalidates the packed images
    with torch.no_grad():
        mod.proj_out.bias.add_(1.0)
        moved = mod(xd, cd)
    np.testing.assert_allclose(N(moved), N(got) + 1.0, rtol=0, atol=1e-5 * scale)
    transformer_cm.USE_SINKS = True


def test_unet_forward_has_no_library_attention_or_gemm(cuda):
    """The whole UNet forward at a reduced spatial size: HIP transformer path == library path (fp32 both), and the
    profiler of the HIP run lists no library attention / GEMM kernel (names `attn_fwd`, `Cijk_`)."""
    from mvip_nerf_amd.guidance import sd_nets
    torch.manual_seed(0)
    unet = sd_nets.UNet2DConditionModel().to(cuda).eval()
    for p in unet.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 9, 64, 64, device=cuda)
    ctx = torch.randn(2, 77, 768, device=cuda)
    t = torch.tensor(417, device=cuda)
    old1x1 = sd_nets.USE_MFMA_CONV1X1
    with torch.no_grad():
        sd_nets.USE_HIP_TRANSFORMER = sd_nets.USE_HIP_TIME_LINEARS = sd_nets.USE_MFMA_CONV1X1 = False
        try:
            ref = unet(x, t, encoder_hidden_states=ctx)[0]
        finally:
            sd_nets.USE_HIP_TRANSFORMER = sd_nets.USE_HIP_TIME_LINEARS = True
            sd_nets.USE_MFMA_CONV1X1 = old1x1
        unet(x, t, encoder_hidden_states=ctx)                      # warm-up: packs weights, caches prompt k/v
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            got = unet(x, t, encoder_hidden_states=ctx)[0]
            torch.cuda.synchronize()
    np.testing.assert_allclose(N(got), N(ref), rtol=0, atol=2e-4 * float(ref.abs().max()))
    names = [e.key for e in prof.key_averages()]
    assert any('attn_f16x3_kernel' in n for n in names)
    assert not [n for n in names if 'attn_fwd' in n or 'Cijk_' in n], names        # no library attention, no library GEMM


@pytest.mark.parametrize('cfg', [0, 1, 2, 3, 4, 5])
def test_gemm_tile_configs_vs_fp64(cuda, cfg):
    """Every workgroup-tile variant of the split-precision GEMM (csrc/gemm_f16x3.hip) against W X in fp64, with bias,
    per-sample channel addend and residual, K from one to many 32-deep stages (pipeline prologue / tail)."""
    from mvip_nerf_amd import ops
    gen = torch.Generator().manual_seed(20 + cfg)
    old = ops.GEMM_CFG
    ops.GEMM_CFG = cfg
    try:
        for Nb, M, K, P in ((2, 128, 32, 256), (1, 256, 64, 512), (2, 384, 320, 256), (1, 128, 96, 1024), (1, 1152, 320, 512)):
            W = torch.randn(M, K, generator=gen) / K ** 0.5
            x = torch.randn(Nb, K, P, generator=gen) * 1.5
            b, ca, rs = torch.randn(M, generator=gen), torch.randn(Nb, M, generator=gen), torch.randn(Nb, M, P, generator=gen)
            ref = torch.einsum('mk,nkp->nmp', W.double(), x.double()) + b.double()[None, :, None] + ca.double()[:, :, None] + rs.double()
            xd = x.to(cuda)
            xs, s2 = ops._scaled_planes(xd, Nb, K, P, K * P, P, 1)
            y = ops.gemm_f16x3(xs, ops.gemm_pack_a(W.to(cuda), M, K, K, 1), Nb, K, M, P, bias=b.to(cuda),
                               chan_add=ca.to(cuda), residual=rs.to(cuda), x_scale2=s2)
            np.testing.assert_allclose(N(y), ref.float().numpy(), rtol=0, atol=3e-6 * float(ref.abs().max()),
                                       err_msg=f'cfg {cfg} shape {(Nb, M, K, P)}')
    finally:
        ops.GEMM_CFG = old


def test_gemm_random_shapes_vs_fp64(cuda):
    """The library's own choice of GEMM kernel (register-streaming kernel, split-K where it applies) on 40 random shapes
    -- every prologue / tail length of the 16-k pipeline, one and two row tiles, with and without the epilogue terms --
    against W X in fp64."""
    from mvip_nerf_amd import ops
    rs = np.random.RandomState(11)
    gen = torch.Generator().manual_seed(11)
    for case in range(40):
        Nb = int(rs.choice([1, 2, 3]))
        M = 32 * int(rs.randint(1, 17))
        K = 32 * int(rs.randint(1, 49))
        P = 256 * int(rs.choice([1, 2, 3]))
        W = torch.randn(M, K, generator=gen) / K ** 0.5
        x = torch.randn(Nb, K, P, generator=gen) * float(rs.choice([1e-3, 1.0, 40.0]))
        bias = torch.randn(M, generator=gen) if rs.rand() < 0.5 else None
        ca = torch.randn(Nb, M, generator=gen) if rs.rand() < 0.3 else None
        res = torch.randn(Nb, M, P, generator=gen) if rs.rand() < 0.5 else None
        ref = torch.einsum('mk,nkp->nmp', W.double(), x.double())
        if bias is not None:
            ref = ref + bias.double()[None, :, None]
        if ca is not None:
            ref = ref + ca.double()[:, :, None]
        if res is not None:
            ref = ref + res.double()
        xd = x.to(cuda)
        xs, s2 = ops._scaled_planes(xd, Nb, K, P, K * P, P, 1)
        y = ops.gemm_f16x3(xs, ops.gemm_pack_a(W.to(cuda), M, K, K, 1), Nb, K, M, P,
                           bias=None if bias is None else bias.to(cuda), chan_add=None if ca is None else ca.to(cuda),
                           residual=None if res is None else res.to(cuda), x_scale2=s2)
        np.testing.assert_allclose(N(y), ref.float().numpy(), rtol=0, atol=4e-6 * float(ref.abs().max()),
                                   err_msg=f'case {case}: N={Nb} M={M} K={K} P={P}')


@pytest.mark.parametrize('C,heads,H,W', [(320, 8, 16, 16), (1280, 8, 8, 8)])
def test_transformer2d_fp16_mode_vs_fp64(cuda, C, heads, H, W):
    """The whole Transformer2DModel in the single-product arithmetic (ops.precision(1): the reference's --fp16 mode on the
    hand-written kernels) vs the fp64 module: fp16-grade (5e-3 of the output scale through eleven chained contractions and
    two softmaxes), and measurably not the split-precision result."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.guidance import sd_nets, transformer_cm
    torch.manual_seed(C + H)
    mod = sd_nets.Transformer2DModel(C, heads, 768).eval()
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.half().float())
    for p in mod.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, C, H, W) * 1.5
    ctx = torch.randn(2, 77, 768)
    with torch.no_grad():
        ref = mod.double()(x.double(), ctx.double())
    mod = mod.float().to(cuda)
    with torch.no_grad():
        full = mod(x.to(cuda), ctx.to(cuda))
        mod.__dict__.pop('_mvip_cm', None)                     # the prompt planes are cached per arithmetic
        with ops.precision(1):
            got = mod(x.to(cuda), ctx.to(cuda))
    scale = float(ref.abs().max())
    e16 = float((got.cpu().double() - ref).abs().max()) / scale
    e32 = float((full.cpu().double() - ref).abs().max()) / scale
    assert e32 < 1e-5 and 1e-5 < e16 < 5e-3, (e32, e16)


@pytest.mark.parametrize('heads,D,Lq,Lk', [(8, 40, 256, 256), (8, 80, 256, 256), (8, 160, 64, 77), (8, 40, 4096, 4096)])
def test_attention_fp16_mode_vs_fp64(cuda, heads, D, Lq, Lk):
    from mvip_nerf_amd import ops
    with ops.precision(1):
        err, got, ref = _attention_case(cuda, 2, heads, D, Lq, Lk, None, seed=5)
    assert 1e-5 < err < 2e-3, err
