"""The pack kernels of the NeRF MLP (csrc/mlp_image.h) against the numpy restatement of the images (mlp_image_numpy.py),
bit for bit: the four forward images, the gradient unpack, the three transposed images.  The same file passes against the
library from before the layouts had one definition (MVIP_LIB_PATH): the bytes are the format."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.weights import seeded_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_image_numpy as M              # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = [11, 12]
T_WORDS = 2176 * 256
_cache = {}


def host_params(seed):
    from mvip_nerf_amd import ops
    if seed not in _cache:
        sd = seeded_state_dict(seed)
        _cache[seed] = [np.ascontiguousarray(sd[k], np.float32) for k in ops.PARAM_ORDER]
    return _cache[seed]


def reference(seed, fmt):
    if (seed, fmt) not in _cache:
        _cache[seed, fmt] = M.forward_image(fmt, host_params(seed))
    return _cache[seed, fmt]


def dev_params(seed, dev):
    return [torch.from_numpy(p).to(dev) for p in host_params(seed)]


def words(t):
    return t.detach().cpu().numpy().view(np.uint32)


def assert_same_words(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{what}: {bad.size} of {got.size} words differ, first at {bad[:4]}: {got[bad[:4]]} != {want[bad[:4]]}'


def pack(fmt, ps):
    from mvip_nerf_amd import ops
    packed = ops.mlp_pack(ps)
    if fmt == 'frag32':
        return packed
    if fmt == 'frag16':
        return ops.plain16(ops.mlp_pack16(ps, packed, fold=False))
    return ops.mlp_pack_f16x3(ps, packed) if fmt == 'h32' else ops.mlp_pack_f16x3_w16(ps, packed)


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('fmt', ['frag32', 'frag16', 'h32', 'h16'])
def test_forward_image_bits(cuda, fmt, seed):
    img = pack(fmt, dev_params(seed, cuda))
    assert img.numel() == M.PACKED_FLOATS
    assert_same_words(words(img), reference(seed, fmt), f'{fmt} image, seed {seed}')


def test_unpack_grads_bits(cuda):
    from mvip_nerf_amd import ops
    image = np.arange(1, M.PACKED_FLOATS + 1, dtype=np.float32)          # distinct values, exact in fp32
    grads = ops.mlp_unpack_grads(torch.from_numpy(image).to(cuda), None)
    for i, (g, want) in enumerate(zip(grads, M.unpack_grads(image))):
        assert_same_words(words(g), want, f'gradient tensor {i}')


def transposed_after_backward(dev, seed, precision):
    """The transposed image one backward of 128 points at tile_points = 128 leaves at the head of its workspace."""
    from mvip_nerf_amd import ops
    from mvip_nerf_amd._lib import call, ptr, ptr_array, stream
    ps = dev_params(seed, dev)
    image = pack('h32' if precision == 1 else 'frag32', ps)
    g = torch.Generator().manual_seed(seed)
    pts, dirs = torch.rand(128, 3, generator=g).to(dev), torch.nn.functional.normalize(torch.randn(128, 3, generator=g)).to(dev)
    d_raw = (torch.randn(128, 4, generator=g) * 1e-3).to(dev)
    ws = ops._workspace(dev, 128)
    ws[:T_WORDS].zero_()
    grads = ops._zero_grads(dev)
    call('mvip_mlp_backward_points', ptr(image), ptr(pts), ptr(dirs), 128, ptr(d_raw), ptr_array(grads), ptr(ws), 128, precision,
         stream())
    return words(ws[:T_WORDS])


def delta16_selected():
    """What the library reads once per process: MVIP_DELTA16 unset or a non-zero integer selects the 16-point delta kernel."""
    e = os.environ.get('MVIP_DELTA16')
    m = re.match(r'\s*[+-]?\d+', e or '')
    return e is None or (m is not None and int(m.group()) != 0)


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('precision', [0, 1])
def test_transposed_image_bits(cuda, precision, seed):
    fp32 = 'frag16' if delta16_selected() else 'frag32'
    fmt, fwd = ('h32', 'h32') if precision == 1 else (fp32, 'frag32')
    want = M.transposed_image(fmt, fwd, reference(seed, fwd))
    assert_same_words(transposed_after_backward(cuda, seed, precision), want, f'transposed {fmt} image, seed {seed}')


def test_transposed_image_bits_32_point_delta(cuda, tmp_path):
    """The 32-point fp32 transposed image: only MVIP_DELTA16=0 selects it, read once per process -- so a fresh child."""
    out = tmp_path / 't32.npy'
    code = ('import sys, numpy as np, torch; sys.path.insert(0, sys.argv[1]); import test_mlp_image as t; '
            'np.save(sys.argv[2], t.transposed_after_backward(torch.device("cuda:0"), t.SEEDS[0], 0))')
    env = dict(os.environ, MVIP_DELTA16='0', PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, '-c', code, os.path.dirname(os.path.abspath(__file__)), str(out)], env=env, check=True,
                   timeout=120)
    want = M.transposed_image('frag32', 'frag32', reference(SEEDS[0], 'frag32'))
    assert_same_words(np.load(out), want, 'transposed frag32 image')
