"""The numpy restatement of the MLP weight images (mlp_image_numpy.py) checked against itself: every parameter element once,
zeros in the padding, decode a bijection, transposed images two ways.  tests/test_mlp_image.py holds the pack kernels
to it bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_image_numpy as M              # noqa: E402


def tagged_params():
    """Every element of the 24 tensors a distinct positive integer below 2^24 (exact in fp32)."""
    out, at = [], 1
    for s in M.PARAM_SHAPES:
        n = int(np.prod(s))
        out.append(np.arange(at, at + n, dtype=np.float32).reshape(s))
        at += n
    assert at < 1 << 24
    return out


@pytest.fixture(scope='module')
def random_params():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32) for s in M.PARAM_SHAPES]


def test_table_matches_the_abi_sizes():
    assert M.SEC_A_FLOATS == 593920 and M.PACKED_FLOATS == 597248
    assert sum(w.shape[0] * w.shape[1] for w in M.transposed_layers(
        [np.zeros((M.PARAM_SHAPES[p][0], len(c))) for p, c in M.LAYERS])) == 2176 * 256


@pytest.mark.parametrize('fmt', ['frag32', 'frag16'])
def test_fp32_images_hold_every_element_once_and_zero_padding(fmt):
    params = tagged_params()
    img = M.forward_image(fmt, params)
    assert img.size == M.PACKED_FLOATS
    tags = np.sort(img[img != 0])
    want = np.sort(np.concatenate([p.ravel() for p in params]))
    np.testing.assert_array_equal(tags, want)                       # all 24 tensors, each element exactly once
    n_real = sum(int(np.prod(s)) for s in M.PARAM_SHAPES)
    assert (img == 0).sum() == M.PACKED_FLOATS - n_real              # and every other slot is a zero


@pytest.mark.parametrize('fmt', ['h32', 'h16'])
def test_fp16_images_hold_every_weight_once_and_zero_padding(fmt):
    # two passes per layer with tags that are exact in fp16 (hi = tag, lo = 0): 1 + row, then 1 + column.  The pair of
    # tags at one image position names one tensor element; every element must turn up at exactly one position.
    F = M.FORMATS[fmt]
    for layer, (p, cols) in enumerate(M.LAYERS):
        units, width = M.PARAM_SHAPES[p]
        images = []
        for tag in (1 + np.arange(units)[:, None] + 0 * np.arange(width), 1 + np.arange(width) + 0 * np.arange(units)[:, None]):
            params = [np.zeros(s, np.float32) for s in M.PARAM_SHAPES]
            params[p] = tag.astype(np.float32)
            el = M.layer_elements(F, M.padded(params, layer)).reshape(-1, 2, 512)      # [k-step][hi | lo][512]
            assert not el[:, 1].any()
            images.append(el[:, 0].astype(np.int64).ravel())
        r, c = images
        assert ((r == 0) == (c == 0)).all()                            # padding is zero in both passes
        assert (r == 0).sum() == units * len(cols) - units * width
        element = (r[r != 0] - 1) * width + (c[c != 0] - 1)
        np.testing.assert_array_equal(np.sort(element), np.arange(units * width))


@pytest.mark.parametrize('fmt', sorted(M.FORMATS))
@pytest.mark.parametrize('K', [64, 128, 256, 288, 320])
def test_decode_is_a_bijection(fmt, K):
    """Every (row, k, lo) of a layer sits at exactly one element, so decode has an inverse -- the index() of csrc/mlp_image.h,
    which the transposed packs read through and tests/test_mlp_image.py therefore checks on the device."""
    F = M.FORMATS[fmt]
    units, terms = (128 if K == 288 else 256), (2 if F.dtype == np.float16 else 1)
    row, k, lo = F.decode(np.arange(units * K * terms), K)
    assert row.min() == 0 and row.max() == units - 1 and k.min() == 0 and k.max() == K - 1 and lo.max() == terms - 1
    np.testing.assert_array_equal(np.sort((row * K + k) * terms + lo), np.arange(units * K * terms))
    x = M.index_table(F, units, K)
    assert (x >= 0).all()
    if terms == 2:                                                     # the lo term of the same weight is one block further on
        assert (lo[x + F.block] == 1).all()
        np.testing.assert_array_equal(row[x + F.block], row[x])
        np.testing.assert_array_equal(k[x + F.block], k[x])


@pytest.mark.parametrize('fmt,fwd', [('frag32', 'frag32'), ('frag16', 'frag32'), ('h32', 'h32')])
def test_transposed_image_is_the_forward_image_of_the_transposed_layers(fmt, fwd, random_params):
    F, S = M.FORMATS[fmt], M.FORMATS[fwd]
    got = M.transposed_image(fmt, fwd, M.forward_image(fwd, random_params))
    assert got.size == 2176 * 256
    mats = [M.padded(random_params, l) for l in range(len(M.LAYERS))]
    if S.dtype == np.float16:            # what the forward image's hi + lo gives, not the fp32 weight itself
        mats = [np.add(*[h.astype(np.float32) for h in M.split(w)]) for w in mats]
    want = np.concatenate([M.layer_elements(F, np.ascontiguousarray(t)) for t in M.transposed_layers(mats)])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    if S.dtype == np.float16:            # and hi + lo of the transposed image reproduces those sums
        at = 0
        for t in M.transposed_layers(mats):
            back = M.layer_values(F, got.view(np.float16)[at:at + 2 * t.size], *t.shape)
            np.testing.assert_array_equal(back, t)
            at += 2 * t.size


def test_unpack_inverts_pack():
    params = tagged_params()
    back = M.unpack_grads(M.forward_image('frag32', params))
    for a, b in zip(back, params):
        np.testing.assert_array_equal(a, b)
