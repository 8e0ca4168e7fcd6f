"""numpy restatement of the NeRF MLP's weight images (csrc/mlp_image.h): a layer table plus four fragment maps.  A helper of
test_mlp_image_cpu.py (which checks it against itself) and test_mlp_image.py (which checks the pack kernels against it bit
for bit); not collected.

An image is [section A: the layers' weights, layer after layer, as 1-KB MFMA operand blocks | section B: small vectors].
The images differ only in the fragment map: where the element for output row `row` and input unit `k` sits in its layer."""
import numpy as np

PARAM_SHAPES = [s for i in range(8) for s in (((256, 63 if i == 0 else 319 if i == 5 else 256)), (256,))] + \
               [(128, 283), (128,), (256, 256), (256,), (1, 256), (1,), (3, 128), (3,)]
P_WV, P_BV, P_WF, P_BF, P_WA, P_BA, P_WR, P_BR = 16, 17, 18, 19, 20, 21, 22, 23

# ---- the stream's layers: (parameter index, real column of each padded k or -1 for a zero) ----------------------------
_r = lambda a, b: list(range(a, b))
LAYERS = [(0, _r(0, 63) + [-1])] + [(2 * l, _r(0, 256)) for l in (1, 2, 3, 4)] + \
         [(10, _r(0, 63) + [-1] + _r(63, 319))] + [(12, _r(0, 256)), (14, _r(0, 256)), (P_WF, _r(0, 256)),
                                                   (P_WV, _r(0, 283) + [-1] * 5)]
SEC_A_FLOATS = sum(PARAM_SHAPES[p][0] * len(c) for p, c in LAYERS)            # 593,920
SEC_B_FLOATS = 13 * 256
PACKED_FLOATS = SEC_A_FLOATS + SEC_B_FLOATS
SECTION_B = [(2 * l + 1, 256 * l) for l in range(8)] + [(P_BF, 2048), (P_BV, 2304), (P_WA, 2432), (P_BA, 2688), (P_WR, 2692),
                                                        (P_BR, 3076)]            # (parameter, float offset), natural order


def padded(params, layer):
    """W[units, padded K] of a stream layer, zeros where the image is padded."""
    p, cols = LAYERS[layer]
    cols = np.asarray(cols)
    w = np.zeros((PARAM_SHAPES[p][0], len(cols)), np.float32)
    w[:, cols >= 0] = np.asarray(params[p], np.float32)[:, cols[cols >= 0]]
    return w


def transposed_layers(mats):
    """The delta kernels' stream: W^T of the view layer's 256 feature inputs, of feature, of layers 7, 6, 5 (h4 part), 4..1."""
    return [mats[9][:, :256].T, mats[8].T, mats[7].T, mats[6].T, mats[5][:, 64:].T] + [mats[l].T for l in (4, 3, 2, 1)]


# ---- the four fragment maps ---------------------------------------------------------------------------------------------
# decode(x, K) -> (row, k, lo) for element x of a layer with padded width K.  Where an element is READ (the transposed packs
# read the forward image) the inverse is needed: index_table() below inverts decode by construction.
class Frag32:
    """fp32, 32x32x2 MFMA: lane (i, h) of block (tile ti, k-group kg) holds W[32 ti + i][8 kg + 4 h + s] at h*128 + i*4 + s;
    the blocks of tiles (2P, 2P + 1) alternate k-group by k-group."""
    dtype, block = np.float32, 256

    @staticmethod
    def decode(x, K):
        local, e = x // 256, x % 256
        pair, rem = local // (2 * (K // 8)), local % (2 * (K // 8))
        return 32 * (2 * pair + rem % 2) + e % 128 // 4, 8 * (rem // 2) + 4 * (e // 128) + e % 4, 0 * x



class Frag16:
    """fp32, 16x16x4 MFMA: block (out tile to, in tile ti), tile by tile; lane (m, g) holds W[16 to + m][16 ti + 4 g + 0..3]."""
    dtype, block = np.float32, 256

    @staticmethod
    def decode(x, K):
        local, lane, s = x // 256, x % 256 // 4, x % 4
        return 16 * (local // (K // 16)) + lane % 16, 16 * (local % (K // 16)) + 4 * (lane // 16) + s, 0 * x



class FragH32:
    """fp16 hi | lo, 32x32x16 MFMA: blocks (tile ti, k-step ks, hi | lo); element j of lane (i, h) is
    W[32 ti + i][16 ks + 8 (j >> 2) + 4 h + (j & 3)]."""
    dtype, block = np.float16, 512

    @staticmethod
    def decode(x, K):
        local, lane, j = x // 512, x % 512 // 8, x % 8
        pair = local // 2
        return 32 * (pair // (K // 16)) + lane % 32, 16 * (pair % (K // 16)) + 8 * (j // 4) + 4 * (lane // 32) + j % 4, local % 2



class FragH16:
    """fp16 hi | lo, 16x16x32 MFMA: blocks (tile to, k-step s, hi | lo); element j of lane (m, g) is W[16 to + m][32 s + U(g, j)],
    U(g, j) = 4 g + j for j < 4 and 16 + 4 g + (j - 4) for j >= 4."""
    dtype, block = np.float16, 512

    @staticmethod
    def decode(x, K):
        local, lane, j = x // 512, x % 512 // 8, x % 8
        pair, g = local // 2, lane // 16
        return 16 * (pair // (K // 32)) + lane % 16, 32 * (pair % (K // 32)) + 16 * (j // 4) + 4 * g + j % 4, local % 2



FORMATS = {'frag32': Frag32, 'frag16': Frag16, 'h32': FragH32, 'h16': FragH16}


def split(w):
    hi = w.astype(np.float16)
    return hi, (w - hi.astype(np.float32)).astype(np.float16)


def layer_elements(F, w):
    """One layer's blocks in format F from its padded matrix w[units, K] (fp16: hi = f16(w), lo = f16(w - hi))."""
    n = w.size * (2 if F.dtype == np.float16 else 1)
    row, k, lo = F.decode(np.arange(n), w.shape[1])
    if F.dtype == np.float32:
        return w[row, k]
    hi, low = split(w)
    return np.where(lo == 1, low[row, k], hi[row, k])


def index_table(F, units, K):
    """x[row, k]: the (hi) element of a layer that holds W[row][k]; the lo term sits F.block further on."""
    n = units * K * (2 if F.dtype == np.float16 else 1)
    row, k, lo = F.decode(np.arange(n), K)
    x = np.full((units, K), -1)
    x[row[lo == 0], k[lo == 0]] = np.flatnonzero(lo == 0)
    return x


def layer_values(F, elems, units, K):
    """The inverse: w[units, K] as fp32 read back element by element (fp16: hi + lo, exact in fp32)."""
    x = index_table(F, units, K)
    return elems[x] if F.dtype == np.float32 else elems[x].astype(np.float32) + elems[x + F.block].astype(np.float32)


def section_b(params):
    b = np.zeros(SEC_B_FLOATS, np.float32)
    for p, off in SECTION_B:
        v = np.asarray(params[p], np.float32).ravel()
        b[off:off + v.size] = v
    return b


def forward_image(fmt, params):
    """The whole image as PACKED_FLOATS fp32 words (fp16 section A viewed as fp32 words)."""
    F = FORMATS[fmt]
    a = np.concatenate([layer_elements(F, padded(params, l)) for l in range(len(LAYERS))])
    return np.concatenate([a.view(np.float32), section_b(params)])


def transposed_image(fmt, fwd_fmt, image):
    """The transposed stream in format `fmt` as its pack kernel forms it: every weight read back from the forward image
    `image` (format fwd_fmt) and, for fp16, split again.  2176 * 256 fp32 words."""
    F, S = FORMATS[fmt], FORMATS[fwd_fmt]
    a = image[:SEC_A_FLOATS].view(S.dtype)
    mats, at = [], 0
    for p, cols in LAYERS:
        units, K = PARAM_SHAPES[p][0], len(cols)
        n = units * K * (2 if S.dtype == np.float16 else 1)
        mats.append(layer_values(S, a[at:at + n], units, K))
        at += n
    return np.concatenate([layer_elements(F, np.ascontiguousarray(t)) for t in transposed_layers(mats)]).view(np.float32)


def unpack_grads(image):
    """The gradient unpack: a frag32 image's real slots scattered back to the 24 tensors (padding slots are dropped)."""
    image = np.asarray(image, np.float32)
    grads = [np.zeros(s, np.float32) for s in PARAM_SHAPES]
    at = 0
    for p, cols in LAYERS:
        units, K, cols = PARAM_SHAPES[p][0], len(cols), np.asarray(cols)
        row, k, _ = Frag32.decode(np.arange(units * K), K)
        real = cols[k] >= 0
        grads[p][row[real], cols[k][real]] = image[at:at + units * K][real]
        at += units * K
    for p, off in SECTION_B:
        grads[p][...] = image[SEC_A_FLOATS + off:SEC_A_FLOATS + off + grads[p].size].reshape(grads[p].shape)
    return grads
