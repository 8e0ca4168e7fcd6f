"""TEST HELPER, not collected: inputs, fp64 references and tolerances of tests/test_hashgrid_model.py (GPU) and
tests/test_hashgrid_model_cpu.py: the hash-grid model NeRF_TCNN -- gather, SH4, five bias-free layers -- restated with
oracle/hashgrid_oracle.py (grid_encode, sh4, the layer algebra of nerf_tcnn_forward) and evaluated in a chosen dtype, forward
and, by torch autograd, every parameter gradient.

Tolerance rule.  A worst-case running bound through five layers is four orders above the actual fp32 error, so the
tolerance is measured on the reference alone: the same oracle evaluated once more in fp32 (tables, weights, sums) gives, per
output column or gradient tensor, E32 = max |oracle32 - oracle64|, and every element of the kernel's result must be within
MARGIN * E32.  The kernels form the same fp32 products in another order (k in pairs through the MFMA, a permuted k, slab
sums), so their error has oracle32's distribution; the CPU module re-sums oracle32 in permuted pairs of k and asserts that this
moves no column or tensor beyond MARGIN / 2 * E32.  E32 is the maximum of a sample, so it needs one: runs at small point
counts (1, 31, ..) are PREFIXES of a 300-point (sh4: 257-point) case and use that case's E32.

Lattice tables (levels with integer scales, points x = j / 128: positions and corner weights exact in fp32, so the kernel's
cells are the reference's): POW2 = gradient_cases.lattice_levels(); ODD = the same scales with hashed levels of
non-power-of-two size (the `hsh % size` fork of hgf_corners).  Module cases run NeRF_TCNN's own table at bound = 100 with
positions formed in fp32 exactly as hg_cell forms them (grid_encode on float32 x01 with a float64 table), fp64 after that."""
import functools

import numpy as np
import torch

import gradient_cases as G
from oracle import hashgrid_oracle as HO

MARGIN = 8
GUARD = 1e-4                         # |hidden pre-activation| >= GUARD * max|z| of its layer, in fp64 (gradient cases)
M32 = 0xFFFFFFFF

# the hashed levels (5, 6, 8 .. 15) capped at multiples of 8 that are no power of two; dense levels as in LATTICE_CAPS:
# level 0 has size == res^3 (8), level 1 size 32 > res^3 = 27
ODD_CAPS = (8, 32, 64, 512, 4096, 4104, 4104, 68928, 65544, 65544, 4104, 65544, 4104, 131080, 4104, 65544)
TABLES = ('POW2', 'ODD')
LATTICE_BASE = 300                   # P <= LATTICE_BASE: prefixes of this case
LATTICE_BIG = 65573                  # 512 workgroups x 4 waves x 32 points = 65536 per sweep of the persistent loop, + a ragged tile
LATTICE_PS = (1, 31, 32, 33, 300, LATTICE_BIG)
SPECIAL_J = ((128, 128, 128), (0, 0, 0), (64, 64, 64), (64, 0, 128))
N_OUT_OF_BOX = 16
NONFINITE_P, NONFINITE_ROW = 70, 37  # three tiles, the last ragged; the replaced point sits in the second
MODULE_PS = (300, 4389)              # one ragged backward tile (padded to 320 for skinny_wgrad); two tiles + a ragged 256-block
MODULE_SEED = 12                     # the fixed rows pass the ReLU guard at both point counts (seeds 1-11 do not)
MODULE_BOUND = 100.0
SH_BASE = 257
SH_PS = (1, 255, 256, 257)
GRAD_NAMES = ('W1', 'W2', 'C1', 'C2', 'C3', 'table')


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _np(t):
    return t.detach().numpy()


# ---------------------------------------------------------------------------------------------- level tables
@functools.lru_cache(maxsize=None)
def lattice_levels(name):
    """[16,4] int32 words {scale (fp32 bits), resolution, offset, size} and the entry count of table POW2 or ODD."""
    if name == 'POW2':
        return G.lattice_levels()
    rows, offset = [], 0
    for scale, cap in zip(G.LATTICE_SCALES, ODD_CAPS):
        res = scale + 1
        size = min((res ** 3 + 7) // 8 * 8, cap)
        rows.append((int(np.float32(scale).view(np.int32)), res, offset, size))
        offset += size
    levels = np.array(rows, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(16, 4)
    _freeze(levels)
    return levels, offset


def dense_levels(levels):
    u = levels.view(np.uint32).astype(np.int64)
    return [l for l in range(16) if u[l, 1] ** 3 <= u[l, 3]]


def dense_wrap_rows(j, levels):
    """Rows of j [P,3] (x = j / 128) of which some corner on some dense level has c.x + c.y res + c.z res^2 (uint32) at or
    beyond the level's size -- the `idx >= size -> idx %= size` branch of hgf_corners.  -> bool [P]."""
    u = levels.view(np.uint32).astype(np.int64)
    hit = np.zeros(len(j), bool)
    for l in dense_levels(levels):
        scale, res, size = int(G.LATTICE_SCALES[l]), u[l, 1], u[l, 3]
        cell = np.floor_divide(j.astype(np.int64) * scale + 64, 128)              # floor(x scale + 0.5)
        for k in range(8):
            c = [(cell[:, d] + ((k >> d) & 1)) & M32 for d in range(3)]
            idx = (c[0] + ((c[1] * res) & M32) + ((c[2] * ((res * res) & M32)) & M32)) & M32
            hit |= idx >= size
    return hit


# ---------------------------------------------------------------------------------------------- the model in a dtype
def mlp_weights(seed):
    """(sigma_net.params [3072], color_net.params [7168]) float32, each matrix by the model's own Xavier rule."""
    from mvip_nerf_amd.run_nerf_helpers_tcnn import _xavier
    gen = torch.Generator().manual_seed(seed)
    sp = torch.cat([_xavier(gen, 64, 32).reshape(-1), _xavier(gen, 16, 64).reshape(-1)])
    cp = torch.cat([_xavier(gen, 64, 32).reshape(-1), _xavier(gen, 64, 64).reshape(-1), _xavier(gen, 16, 64).reshape(-1)])
    return sp, cp


def matrices(sp, cp):
    """NeRF_TCNN.mlp_matrices on flat parameter vectors: W1 [64,32], W2 [16,64], C1 [64,32], C2 [64,64], C3 [16,64]."""
    return (sp[:2048].view(64, 32), sp[2048:3072].view(16, 64),
            cp[:2048].view(64, 32), cp[2048:6144].view(64, 64), cp[6144:7168].view(16, 64))


def split_table(table, levels, dtype, requires_grad=False):
    """table [n,2] -> one tensor per level in `dtype` (separate autograd leaves: a gather's gradient then has the size of its
    level, not of the whole table)."""
    u = levels.view(np.uint32).astype(np.int64)
    return [table[u[l, 2]:u[l, 2] + u[l, 3]].to(dtype).clone().requires_grad_(requires_grad) for l in range(16)]


def encode(x01, tables, levels, unit_weights=False):
    """HO.grid_encode level by level on the per-level tables -> [P,32]."""
    out = []
    for l in range(16):
        row = np.array(levels[l:l + 1])
        row[0, 2] = 0
        out.append(HO.grid_encode(x01, tables[l], row, unit_weights))
    return torch.cat(out, -1)


def _pair_order(K):
    return np.random.RandomState(K).permutation(K).reshape(-1, 2)


def _pair_matmul(h, W):
    """h @ W.T summed as the matrix pipe does it, in a permuted order: acc += h[k0] W[k0] + h[k1] W[k1] over pairs of k."""
    acc = None
    for k0, k1 in _pair_order(W.shape[1]):
        t = h[:, int(k0), None] * W[None, :, int(k0)] + h[:, int(k1), None] * W[None, :, int(k1)]
        acc = t if acc is None else acc + t
    return acc


def network(f, dirs, mats, pairs=False):
    """The layer algebra of HO.nerf_tcnn_forward after the encoding, in f's dtype: f [P,32], dirs [P,3] (unit range [-1,1]),
    mats as `matrices` -> out [P,4] = (colour, sigma) and the three hidden pre-activations [P,64]."""
    W1, W2, C1, C2, C3 = mats
    mm = _pair_matmul if pairs else (lambda h, W: h @ W.T)
    z1 = mm(f, W1)
    h = mm(torch.relu(z1), W2)
    cin = torch.cat([HO.sh4((dirs.to(f.dtype) + 1) / 2), h[:, 1:16], torch.ones_like(h[:, :1])], -1)
    z2 = mm(cin, C1)
    z3 = mm(torch.relu(z2), C2)
    c = mm(torch.relu(z3), C3)
    return torch.cat([c[:, :3], h[:, :1]], -1), (z1, z2, z3)


def worst_ratio(got, ref, tol):
    """max of |got - ref| / tol over the elements (tol broadcast; 0 / 0 counts as 0, x / 0 as inf; NaN counts as inf)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ---------------------------------------------------------------------------------------------- fused kernel on the lattice
@functools.lru_cache(maxsize=None)
def lattice_inputs(name, n):
    """n = LATTICE_BASE or LATTICE_BIG.  -> dict: levels, j [n,3] integers (x = j / 128; rows 0-3 SPECIAL_J, rows 4-19 out of
    the box with coordinates in -16..-1 and 129..144, the rest uniform in 0..128), dirs [n,3] float32 unit vectors, table
    [entries,2] ~ N(0,1) float32, sp / cp the Xavier weights."""
    levels, entries = lattice_levels(name)
    rs = np.random.RandomState(6000 + n + TABLES.index(name))
    j = rs.randint(0, 129, size=(n, 3))
    j[:4] = SPECIAL_J
    oob = np.where(rs.uniform(size=(N_OUT_OF_BOX, 3)) < 0.5, rs.randint(-16, 0, size=(N_OUT_OF_BOX, 3)),
                   rs.randint(129, 145, size=(N_OUT_OF_BOX, 3)))
    j[4:4 + N_OUT_OF_BOX] = oob
    d = rs.normal(size=(n, 3))
    dirs = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    table = rs.normal(size=(entries, 2)).astype(np.float32)
    sp, cp = mlp_weights(7 + TABLES.index(name))
    sp, cp = sp.numpy(), cp.numpy()
    _freeze(j, dirs, table, sp, cp)
    return {'levels': levels, 'j': j, 'dirs': dirs, 'table': table, 'sp': sp, 'cp': cp}


@functools.lru_cache(maxsize=None)
def lattice_eval(name, n, dtype, pairs=False):
    """The model on lattice_inputs(name, n) in `dtype` (x = j / 128 is exact in either) -> out [n,4] as float64 values."""
    inp = lattice_inputs(name, n)
    x01 = (torch.from_numpy(inp['j'].copy()).to(torch.float64) / 128.0).to(dtype)
    tables = split_table(torch.from_numpy(inp['table'].copy()), inp['levels'], dtype)
    mats = matrices(torch.from_numpy(inp['sp'].copy()).to(dtype), torch.from_numpy(inp['cp'].copy()).to(dtype))
    with torch.no_grad():
        out, _ = network(encode(x01, tables, inp['levels']), torch.from_numpy(inp['dirs'].copy()), mats, pairs)
    assert out.dtype == dtype
    out = _np(out).astype(np.float64)
    _freeze(out)
    return out


def lattice_base(P):
    return LATTICE_BASE if P <= LATTICE_BASE else LATTICE_BIG


def lattice_reference(name, P):
    """-> (ref [P,4] float64, E32 [4], tol [4] = MARGIN * E32) for the first P rows of the case P belongs to."""
    n = lattice_base(P)
    r64, r32 = lattice_eval(name, n, torch.float64), lattice_eval(name, n, torch.float32)
    E32 = np.abs(r32 - r64).max(0)
    return r64[:P], E32, MARGIN * E32


# ---------------------------------------------------------------------------------------------- the module, bound = 100
@functools.lru_cache(maxsize=None)
def module_model():
    """NeRF_TCNN(seed=MODULE_SEED) on the CPU with encoder.params rescaled to U(-1, 1); the GPU tests move a copy of it."""
    from mvip_nerf_amd.run_nerf_helpers_tcnn import NeRF_TCNN
    net = NeRF_TCNN(seed=MODULE_SEED, bound=int(MODULE_BOUND))
    with torch.no_grad():
        net.encoder.params.mul_(1e4)
    return net


def module_fixed_rows():
    """The six face centres, the eight box corners at +-100 and four points at +-99.99."""
    b, e = MODULE_BOUND, 99.99
    faces = [[s * b if a == d else 0.0 for a in range(3)] for d in range(3) for s in (1, -1)]
    corners = [[sx * b, sy * b, sz * b] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    near = [[e, e, e], [-e, -e, -e], [e, -e, e], [-e, e, 0.0]]
    return np.array(faces + corners + near, dtype=np.float32)


def _module_forward(x, dirs, dtype, pairs=False, tables=None, mats=None):
    """x [P,3] float32 raw coordinates -> out, hidden pre-activations; positions in fp32 as hg_cell forms them."""
    net = module_model()
    levels = net.levels.numpy()
    x01 = torch.from_numpy((x + np.float32(MODULE_BOUND)) / np.float32(2 * MODULE_BOUND))
    assert x01.dtype == torch.float32
    if tables is None:
        tables = split_table(net.encoder.params.detach().reshape(-1, 2), levels, dtype)
        mats = matrices(net.sigma_net.params.detach().to(dtype), net.color_net.params.detach().to(dtype))
    return network(encode(x01, tables, levels), torch.tensor(np.array(dirs)), mats, pairs)


def guard_margin(zs):
    """min over the points of min_units |z| / (GUARD * max|z| of the layer), per point; >= 1 passes.  zs: three [P,64]."""
    r = [np.abs(_np(z)).min(-1) / (GUARD * np.abs(_np(z)).max()) for z in zs]
    return np.minimum(np.minimum(r[0], r[1]), r[2])


@functools.lru_cache(maxsize=None)
def module_inputs(P):
    """-> dict: x [P,3] float32 (rows 0-17 module_fixed_rows, the rest uniform in +-4), dirs [P,3] float32 unit vectors,
    g [P,4] float32 cotangents ~ N(0,1) with all four zero on ~10 % of the points.  Points with a hidden pre-activation within
    GUARD of 0 in fp64 are redrawn (the fixed rows are kept: MODULE_SEED is chosen so that they pass)."""
    rs = np.random.RandomState(8000 + P)
    fixed = module_fixed_rows()
    x = rs.uniform(-4, 4, size=(P, 3)).astype(np.float32)
    x[:len(fixed)] = fixed
    d = rs.normal(size=(P, 3))
    dirs = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    for _ in range(20):
        with torch.no_grad():
            _, zs = _module_forward(x, dirs, torch.float64)
        bad = np.nonzero(guard_margin(zs) < 1.0)[0]
        bad = bad[bad >= len(fixed)]
        if len(bad) == 0:
            break
        x[bad] = rs.uniform(-4, 4, size=(len(bad), 3)).astype(np.float32)
    g = rs.normal(size=(P, 4)).astype(np.float32)
    g[rs.uniform(size=P) < 0.1] = 0
    g[:len(fixed)][g[:len(fixed), 0] == 0] = 1.0                     # the fixed rows always contribute
    _freeze(x, dirs, g)
    return {'x': x, 'dirs': dirs, 'g': g}


@functools.lru_cache(maxsize=None)
def module_eval(P, dtype, pairs=False):
    """The module on module_inputs(P) in `dtype`, loss = (out * g).sum(), gradients by autograd.  -> dict of float64-valued
    arrays: out [P,4], zmargin [P] (guard_margin), masks (three bool [P,64]), W1 .. C3 and table [n,2] (the gradients)."""
    net = module_model()
    inp = module_inputs(P)
    levels = net.levels.numpy()
    tables = split_table(net.encoder.params.detach().reshape(-1, 2), levels, dtype, requires_grad=True)
    sp = net.sigma_net.params.detach().to(dtype).clone().requires_grad_(True)
    cp = net.color_net.params.detach().to(dtype).clone().requires_grad_(True)
    out, zs = _module_forward(inp['x'], inp['dirs'], dtype, pairs, tables, matrices(sp, cp))
    assert out.dtype == dtype
    (out * torch.from_numpy(inp['g'].copy()).to(dtype)).sum().backward()
    gs, gc = matrices(sp.grad, cp.grad)[:2], matrices(sp.grad, cp.grad)[2:]
    res = {'out': _np(out).astype(np.float64), 'zmargin': guard_margin(zs), 'masks': tuple(_np(z) > 0 for z in zs),
           'table': np.concatenate([_np(t.grad) for t in tables]).astype(np.float64)}
    for name, m in zip(GRAD_NAMES[:5], gs + gc):
        res[name] = _np(m).astype(np.float64)
    return res


@functools.lru_cache(maxsize=None)
def module_touched(P):
    """bool [n]: table entries that a corner of a point with a non-zero cotangent lands on."""
    net = module_model()
    inp = module_inputs(P)
    levels = net.levels.numpy()
    u = levels.view(np.uint32).astype(np.int64)
    tables = [torch.zeros(int(u[l, 3]), 2, dtype=torch.float64, requires_grad=True) for l in range(16)]
    x01 = torch.from_numpy((inp['x'] + np.float32(MODULE_BOUND)) / np.float32(2 * MODULE_BOUND))
    live = torch.from_numpy((inp['g'] != 0).any(-1).astype(np.float64))
    (encode(x01, tables, levels, unit_weights=True) * live[:, None]).sum().backward()
    return np.concatenate([_np(t.grad)[:, 0] for t in tables]) > 0


@functools.lru_cache(maxsize=None)
def module_reference(P):
    """-> (r64 = module_eval(P, float64), E32 {name: max |oracle32 - oracle64|} for the four output columns ('out', [4]) and
    the six gradient tensors (scalars))."""
    r64, r32 = module_eval(P, torch.float64), module_eval(P, torch.float32)
    E32 = {'out': np.abs(r32['out'] - r64['out']).max(0)}
    for name in GRAD_NAMES:
        E32[name] = float(np.abs(r32[name] - r64[name]).max())
    return r64, E32


# ---------------------------------------------------------------------------------------------- sh4
@functools.lru_cache(maxsize=None)
def sh_inputs():
    """[SH_BASE,3] float32: +-axes, (1,1,1)/sqrt(3), non-unit vectors and the zero vector first, then random unit vectors."""
    rs = np.random.RandomState(77)
    d = rs.normal(size=(SH_BASE, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    fixed = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [3 ** -0.5] * 3,
             [0.3, -0.2, 0.1], [2.0, -1.0, 0.5], [0, 0, 0], [-0.7, 0.7, 0.7]]
    d[:len(fixed)] = fixed
    d = d.astype(np.float32)
    _freeze(d)
    return d


@functools.lru_cache(maxsize=None)
def sh_reference():
    """-> (ref [SH_BASE,16] float64, E32 [16]): HO.sh4 on the directions widened to fp64, and the fp32 evaluation's distance."""
    d = torch.from_numpy(sh_inputs().copy())
    r64 = _np(HO.sh4((d.double() + 1) / 2))
    r32 = _np(HO.sh4((d + 1) / 2))
    assert r32.dtype == np.float32
    return r64, np.abs(r32.astype(np.float64) - r64).max(0)


SH_ROW0 = np.float32(0.28209479177387814)
