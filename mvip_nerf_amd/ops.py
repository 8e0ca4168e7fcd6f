"""Thin tensor-level wrappers over the C ABI (allocation + autograd plumbing only).

Every function of the NeRF render / training path here launches HIP kernels from libmvipnerf.so on the
current torch stream; inputs must be dense fp32 tensors on the GPU and nothing computes on the CPU.
No library contraction runs anywhere on this path: the hash-grid model's small layers take `csrc/skinny_gemm.hip` for the
forward, the data gradient and the weight gradient (`_LinearCM`; `MVIP_SKINNY_LINEAR=0` switches back to `W @ X` for A/B
timing only), the SDS networks the split-precision kernels.  What stock torch GPU ops remain are tensor allocation,
concatenations and a few elementwise glue ops; they are named where they occur.
"""
import collections
import weakref

import torch

from . import _lib
from ._lib import ptr, stream, call

_F32 = torch.float32


def _f32c(t):
    """Dense fp32 view/copy of a device tensor."""
    if t.dtype != _F32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
# rays
# ------------------------------------------------------------------------------------------------

def get_rays(H, W, focal, c2w, patch=None):
    """(rays_o, rays_d), each [h, w, 3]; `patch` = (i, j, len1, len2) crops rows i.., cols j..
    (DS_NeRF/run_nerf_helpers.py:249-260, DS_NeRF/run.py:1174-1177)."""
    c = _f32c(c2w[:3, :4])
    y0, x0, h, w = (0, 0, H, W) if patch is None else [int(v) for v in patch]
    ro = torch.empty((h, w, 3), device=c.device, dtype=_F32)
    rd = torch.empty_like(ro)
    call('mvip_get_rays', ptr(c), int(H), int(W), float(focal), y0, x0, h, w, ptr(ro), ptr(rd), stream())
    return ro, rd


def ray_rows(rays_o, rays_d, near, far, viewdirs_src=None):
    """[B,3] x2 -> [B,11] rows (o, d, near, far, d/|d|)  (DS_NeRF/run.py:1182-1207)."""
    o, d = _f32c(rays_o.reshape(-1, 3)), _f32c(rays_d.reshape(-1, 3))
    v = None if viewdirs_src is None else _f32c(viewdirs_src.reshape(-1, 3))
    rows = torch.empty((o.shape[0], 11), device=o.device, dtype=_F32)
    call('mvip_ray_rows', ptr(o), ptr(d), ptr(v), float(near), float(far), o.shape[0], ptr(rows), stream())
    return rows


def ray_rows_from_pose(c2w, H, W, focal, near, far, sel=None):
    """Rows for the pixels `sel` (int64 flat y*W+x indices; None = whole frame, raster order)."""
    c = _f32c(c2w[:3, :4])
    if sel is not None:
        sel = sel.to(torch.int64).contiguous()
    B = H * W if sel is None else sel.numel()
    rows = torch.empty((B, 11), device=c.device, dtype=_F32)
    call('mvip_ray_rows_from_pose', ptr(c), int(H), int(W), float(focal), float(near), float(far),
         ptr(sel, torch.int64), B, ptr(rows), stream())
    return rows


_T_VALS = {}


def _t_vals(S, device):
    key = (S, device)
    if key not in _T_VALS:
        _T_VALS[key] = torch.linspace(0., 1., steps=S, device=device, dtype=_F32)
    return _T_VALS[key]


def stratified_z(rows, S, lindisp, t_rand=None):
    """[B,S] sample depths (DS_NeRF/run.py:1759-1781); t_rand [B,S] uniforms or None."""
    B = rows.shape[0]
    z = torch.empty((B, S), device=rows.device, dtype=_F32)
    tr = None if t_rand is None else _f32c(t_rand)
    call('mvip_stratified_z', ptr(rows), rows.shape[1], B, int(S), ptr(_t_vals(S, rows.device)),
         int(bool(lindisp)), ptr(tr), ptr(z), stream())
    return z


def posenc(x, L):
    """Embedder.embed: [..,3] -> [.., 3+6L]."""
    xs = _f32c(x.reshape(-1, 3))
    y = torch.empty((xs.shape[0], 3 + 6 * L), device=xs.device, dtype=_F32)
    call('mvip_posenc', ptr(xs), xs.shape[0], int(L), ptr(y), stream())
    return y.reshape(*x.shape[:-1], 3 + 6 * L)


# ------------------------------------------------------------------------------------------------
# fused MLP
# ------------------------------------------------------------------------------------------------

PARAM_ORDER = tuple([f'pts_linears.{i}.{k}' for i in range(8) for k in ('weight', 'bias')]
                    + [f'{n}.{k}' for n in ('views_linears.0', 'feature_linear', 'alpha_linear', 'rgb_linear')
                       for k in ('weight', 'bias')])
PARAM_SHAPES = tuple([(256, 63), (256,)] + [(256, 256), (256,)] * 4 + [(256, 319), (256,)]
                     + [(256, 256), (256,)] * 2 + [(128, 283), (128,), (256, 256), (256,), (1, 256), (1,),
                                                     (3, 128), (3,)])

_PACKED_FLOATS = None


def packed_floats():
    global _PACKED_FLOATS
    if _PACKED_FLOATS is None:
        _PACKED_FLOATS = int(_lib.load().mvip_mlp_packed_floats())
    return _PACKED_FLOATS


def mlp_pack(params):
    """24 parameter tensors (state-dict order) -> a NEW packed image tensor."""
    ps = [_f32c(p.detach()) for p in params]
    for p, shp in zip(ps, PARAM_SHAPES):
        if tuple(p.shape) != shp:
            raise _lib.MvipError(f'fused MLP is built for the 8x256 NeRF; got parameter shape {tuple(p.shape)} '
                                 f'where {shp} is expected')
    packed = torch.empty(packed_floats(), device=ps[0].device, dtype=_F32)
    call('mvip_mlp_pack', _lib.ptr_array(ps), ptr(packed), stream())
    return packed


_PACKED_FOLD_FLOATS = None


def packed_fold_floats():
    global _PACKED_FOLD_FLOATS
    if _PACKED_FOLD_FLOATS is None:
        _PACKED_FOLD_FLOATS = int(_lib.load().mvip_mlp_packed_fold_floats())
    return _PACKED_FOLD_FLOATS


def mlp_pack16(params, packed_f32, fold=True):
    """Image for the two-waves-per-SIMD kernels (16 points per wave, csrc/mlp_fwd16.hip): the EXTENDED image
    [plain image, packed_floats() | folded view blocks | small vectors with the folded bias] (csrc/mlp_layout.h).  Handed to
    mlp_rays / mlp_points / render_*_fused it selects the folded inference network (feature_linear multiplied into the view
    layer); its head, plain16(img), selects the unfolded one and is what the training forward reads.  fold=False leaves
    the tail unwritten -- mlp_fold_pack16 fills it later -- and such an image must reach the kernels only as plain16(img)."""
    ps = [_f32c(p.detach()) for p in params]
    img = torch.empty(packed_fold_floats(), device=ps[0].device, dtype=_F32)
    call('mvip_mlp_pack16', _lib.ptr_array(ps), ptr(packed_f32), ptr(img), stream())
    if fold:
        call('mvip_mlp_fold_pack16', _lib.ptr_array(ps), ptr(img), stream())
    return img


def mlp_fold_pack16(params, img):
    """Fill the tail of an extended image whose head mlp_pack16 wrote for the same parameters."""
    if img.numel() != packed_fold_floats():
        raise _lib.MvipError('mlp_fold_pack16 needs the extended image of mlp_pack16')
    ps = [_f32c(p.detach()) for p in params]
    call('mvip_mlp_fold_pack16', _lib.ptr_array(ps), ptr(img), stream())
    return img


def plain16(img):
    """The plain (unfolded) image inside an image of mlp_pack16: a view of its first packed_floats() floats."""
    return img[:packed_floats()]


def _fold16(packed16):
    """'_fold' when `packed16` is an extended image (the folded entries run), '' for a plain one."""
    n = packed16.numel()
    if n == packed_fold_floats():
        return '_fold'
    if n != packed_floats():
        raise _lib.MvipError(f'not an image of mlp_pack16: {n} floats')
    return ''


def mlp_pack_f16x3(params, packed_f32):
    """Image for the split-precision forward (precision=1); same size as the fp32 image."""
    ps = [_f32c(p.detach()) for p in params]
    img = torch.empty(packed_floats(), device=ps[0].device, dtype=_F32)
    call('mvip_mlp_pack_f16x3', _lib.ptr_array(ps), ptr(img), ptr(packed_f32), stream())
    return img


def mlp_pack_f16x3_w16(params, packed_f32):
    """Image for the two-waves-per-SIMD split-precision forward (csrc/mlp_fwd16_f16x3.hip); same size as the fp32 image."""
    ps = [_f32c(p.detach()) for p in params]
    img = torch.empty(packed_floats(), device=ps[0].device, dtype=_F32)
    call('mvip_mlp_pack_f16x3_w16', _lib.ptr_array(ps), ptr(packed_f32), ptr(img), stream())
    return img


def mlp_unpack_grads(grad_packed, like):
    grads = [torch.empty(shp, device=grad_packed.device, dtype=_F32) for shp in PARAM_SHAPES]
    call('mvip_mlp_unpack_grads', ptr(grad_packed), _lib.ptr_array(grads), 0, stream())
    return grads


_WORKSPACE = {}
import os as _os
# points per backward tile: delta + weight-gradient launches per tile, 20 KB of G/activation workspace per point (5.2 GB at
# 262,144).  Measured in round 5 on configs[2] / configs[3] iterations (one box, ms): 16,384 points 221 / -, 32,768 175,
# 65,536 156, 131,072 146, 262,144 143.0 / 399.9, 524,288 141.9 / 397.9, 1,048,576 140.9 / 397.0 (the weight-gradient launches
# pay a ramp and a 256 x 256 atomic flush per workgroup and tile); the configs[1] iteration measures the same from 262,144 up.
# The default stays at 262,144: as the default, the 21-GB workspace of 1,048,576 ran tests/test_configs_large.py's replicas
# (several processes on one device beside a 116-GB parent) out of memory.  MVIP_BWD_TILE_POINTS=1048576 buys the 1.5 % on a
# device the job owns.
BWD_TILE_POINTS = int(_os.environ.get('MVIP_BWD_TILE_POINTS', 262144))


def _zero_grads(device):
    """24 zeroed gradient tensors carved from one flat allocation (one memset)."""
    flat = torch.zeros(sum(_numel(s) for s in PARAM_SHAPES), device=device, dtype=_F32)
    out, o = [], 0
    for shp in PARAM_SHAPES:
        n = _numel(shp)
        out.append(flat[o:o + n].view(shp))
        o += n
    return out


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _workspace(device, tile_points):
    key = (device, tile_points)
    if key not in _WORKSPACE:
        n = int(_lib.load().mvip_mlp_backward_workspace_bytes(tile_points))
        _WORKSPACE[key] = torch.empty(max(n, 16) // 4 + 4, device=device, dtype=_F32)
    return _WORKSPACE[key]


# Keep the activations of a training forward for its backward (9.9 KB per point) while they fit the DEVICE: the
# budget (for ALL live stashes together) is computed per call from what is free right now (hipMemGetInfo + the allocator's cached-but-unused blocks),
# so two ranks sharing one device, a resident fp32 SD UNet + VAE, or a smaller-HBM part shrink it by themselves.
# Beyond it -- or if the allocation fails -- the backward recomputes the activations tile by tile.
# MVIP_STASH_BUDGET_BYTES overrides the computed budget (0 = always recompute).
STASH_FREE_FRACTION = 0.6          # of the currently free bytes, after the backward workspace is set aside
_stash_live = {}                   # device index -> bytes of live stashes


_FREE_CACHE = {}                   # device index -> (bytes reserved by torch at query time, free bytes from the driver, time)
# The cached answer also EXPIRES: another process on the device (mvip_nerf_amd/replicas.py with --devices 0,0, any other
# tenant) moves the free memory without touching this process's counters.  MVIP_SHARED_DEVICE=1 (set by replicas.launch
# when several replicas share a device) shortens the lifetime to every query.
FREE_CACHE_SECONDS = 0.0 if _os.environ.get('MVIP_SHARED_DEVICE') == '1' else 0.25


def _device_free_bytes(device):
    """hipMemGetInfo through torch, asked again only when torch's own reservation has changed since the last answer or the
    answer is older than FREE_CACHE_SECONDS: the driver call costs milliseconds once tens of GB are mapped (five stash
    allocations per iteration turned a 54 ms training iteration into 75-94 ms of wall time: tools/train_step_profile.py
    --after-hashgrid), and between two queries the device's free memory moves only when torch itself maps or unmaps memory
    -- which `memory_reserved` (a host-side counter) shows -- or when ANOTHER process does, which only time can cover (the
    allocation itself is guarded as well, see _take_stash)."""
    import time
    key = device.index if device.index is not None else torch.cuda.current_device()
    reserved = torch.cuda.memory_reserved(device)
    now = time.monotonic()
    hit = _FREE_CACHE.get(key)
    if hit is None or hit[0] != reserved or now - hit[2] > FREE_CACHE_SECONDS:
        hit = (reserved, torch.cuda.mem_get_info(device)[0], now)
        _FREE_CACHE[key] = hit
    return hit[1]


def _stash_budget(device):
    env = _os.environ.get('MVIP_STASH_BUDGET_BYTES')
    if env is not None:
        return int(env)
    free = _device_free_bytes(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    ws_bytes = 0 if (device, BWD_TILE_POINTS) in _WORKSPACE else int(
        _lib.load().mvip_mlp_backward_workspace_bytes(BWD_TILE_POINTS))
    # all live stashes together may hold STASH_FREE_FRACTION of what is available to them (free now + already held)
    key = device.index if device.index is not None else torch.cuda.current_device()
    live = _stash_live.get(key, 0)
    return int(STASH_FREE_FRACTION * max(free + live - ws_bytes, 0)) - live


def _take_stash(P, device):
    n = int(_lib.load().mvip_mlp_stash_floats(P))
    if 4 * n > _stash_budget(device):
        return None
    try:
        t = torch.empty(n, device=device, dtype=_F32)
    except torch.OutOfMemoryError:
        return None                                  # fragmentation or a concurrent process: recompute instead
    key = device.index if device.index is not None else torch.cuda.current_device()
    _stash_live[key] = _stash_live.get(key, 0) + 4 * n
    weakref.finalize(t, _stash_freed, key, 4 * n)   # also covers graphs that are dropped without backward
    return t


def _stash_freed(key, nbytes):
    _stash_live[key] = _stash_live.get(key, 0) - nbytes


class _MLPRays(torch.autograd.Function):
    """raw[B,S,4] = MLP(enc(o + d z), enc(viewdir)); gradients flow to the 24 parameters only."""

    @staticmethod
    def forward(ctx, rows, z, packed, precision, packed16, *params):
        """`packed` is the weight image of `precision` (0: fp32 image, 1: f16x3 image); `packed16` (optional) the image of
        the two-waves-per-SIMD kernel of that precision (mlp_pack16 / mlp_pack_f16x3_w16), which then runs the stash-writing
        forward; the backward always works from `packed`."""
        B, S = z.shape
        raw = torch.empty((B, S, 4), device=z.device, dtype=_F32)
        stash = _take_stash(B * S, z.device)
        if stash is None:
            call('mvip_mlp_forward_rays', ptr(packed), ptr(rows), ptr(z), B, S, ptr(raw), precision, stream())
        elif packed16 is not None and precision == 0:
            call('mvip_mlp_forward_rays_stash16', ptr(packed16), ptr(rows), ptr(z), B, S, ptr(raw), ptr(stash), stream())
        elif packed16 is not None and precision == 1:       # the two-wave split-precision kernel (its own image; the backward keeps `packed`)
            call('mvip_mlp_forward_rays_stash_f16x3_w16', ptr(packed16), ptr(rows), ptr(z), B, S, ptr(raw), ptr(stash), stream())
        else:
            call('mvip_mlp_forward_rays_stash', ptr(packed), ptr(rows), ptr(z), B, S, ptr(raw), ptr(stash), precision,
                 stream())
        ctx.save_for_backward(rows, z, packed)
        ctx.stash, ctx.precision = stash, precision
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        rows, z, packed = ctx.saved_tensors
        B, S = z.shape
        grads = _zero_grads(z.device)
        ws = _workspace(z.device, BWD_TILE_POINTS)
        stash, ctx.stash = ctx.stash, None
        if stash is None:
            call('mvip_mlp_backward_rays', ptr(packed), ptr(rows), ptr(z), B, S, ptr(_f32c(d_raw)),
                 _lib.ptr_array(grads), ptr(ws), BWD_TILE_POINTS, ctx.precision, stream())
        else:
            call('mvip_mlp_backward_stash', ptr(packed), ptr(stash), B * S, ptr(_f32c(d_raw)),
                 _lib.ptr_array(grads), ptr(ws), BWD_TILE_POINTS, ctx.precision, stream())
            del stash
        return (None, None, None, None, None, *grads)


class _MLPPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, dirs, packed, precision, *params):
        P = pts.shape[0]
        raw = torch.empty((P, 4), device=pts.device, dtype=_F32)
        call('mvip_mlp_forward_points', ptr(packed), ptr(pts), ptr(dirs), P, ptr(raw), precision, stream())
        ctx.save_for_backward(pts, dirs, packed)
        ctx.precision = precision
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        pts, dirs, packed = ctx.saved_tensors
        grads = _zero_grads(pts.device)
        ws = _workspace(pts.device, BWD_TILE_POINTS)
        call('mvip_mlp_backward_points', ptr(packed), ptr(pts), ptr(dirs), pts.shape[0], ptr(_f32c(d_raw)),
             _lib.ptr_array(grads), ptr(ws), BWD_TILE_POINTS, ctx.precision, stream())
        return (None, None, None, None, *grads)


def mlp_rays(rows, z, packed, params, packed_f16x3=None, train_f16x3=None, packed16=None, train16=None, f16x3_w16=None,
             train_f16x3_w16=None):
    """Fused forward from ray rows + depths.  `params` (the 24 tensors) are passed so autograd
    routes the gradients back to them; with no grad needed the Function is skipped.
    `packed_f16x3` selects the split-precision kernel (precision = 1) for no-grad calls,
    `train_f16x3` (the same kind of image) for calls that will be back-propagated, `packed16` the exact-fp32
    two-waves-per-SIMD inference kernel (no-grad calls at precision 0), `train16` the same image for the stash-writing
    training forward at precision 0, `f16x3_w16` (ops.mlp_pack_f16x3_w16) the two-waves-per-SIMD split-precision kernel
    for no-grad calls (takes precedence over `packed_f16x3`), `train_f16x3_w16` the same kind of image for the stash-writing
    training forward at precision 1 (the backward keeps `train_f16x3`)."""
    rows, z = _f32c(rows), _f32c(z)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        if train_f16x3 is not None:
            return _MLPRays.apply(rows, z, train_f16x3, 1, train_f16x3_w16, *params)
        return _MLPRays.apply(rows, z, packed, 0, train16, *params)
    B, S = z.shape
    raw = torch.empty((B, S, 4), device=z.device, dtype=_F32)
    if f16x3_w16 is not None:
        call('mvip_mlp_forward_rays_f16x3_w16', ptr(f16x3_w16), ptr(rows), ptr(z), B, S, ptr(raw), stream())
    elif packed_f16x3 is not None:
        call('mvip_mlp_forward_rays', ptr(packed_f16x3), ptr(rows), ptr(z), B, S, ptr(raw), 1, stream())
    elif packed16 is not None:
        call('mvip_mlp_forward_rays16' + _fold16(packed16), ptr(packed16), ptr(rows), ptr(z), B, S, ptr(raw), stream())
    else:
        call('mvip_mlp_forward_rays', ptr(packed), ptr(rows), ptr(z), B, S, ptr(raw), 0, stream())
    return raw


def mlp_points(pts, dirs, packed, params, packed_f16x3=None, train_f16x3=None, packed16=None, f16x3_w16=None):
    pts, dirs = _f32c(pts), _f32c(dirs)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        if train_f16x3 is not None:
            return _MLPPoints.apply(pts, dirs, train_f16x3, 1, *params)
        return _MLPPoints.apply(pts, dirs, packed, 0, *params)
    raw = torch.empty((pts.shape[0], 4), device=pts.device, dtype=_F32)
    if f16x3_w16 is not None:
        call('mvip_mlp_forward_points_f16x3_w16', ptr(f16x3_w16), ptr(pts), ptr(dirs), pts.shape[0], ptr(raw), stream())
    elif packed_f16x3 is not None:
        call('mvip_mlp_forward_points', ptr(packed_f16x3), ptr(pts), ptr(dirs), pts.shape[0], ptr(raw), 1, stream())
    elif packed16 is not None:
        call('mvip_mlp_forward_points16' + _fold16(packed16), ptr(packed16), ptr(pts), ptr(dirs), pts.shape[0], ptr(raw), stream())
    else:
        call('mvip_mlp_forward_points', ptr(packed), ptr(pts), ptr(dirs), pts.shape[0], ptr(raw), 0, stream())
    return raw


# ------------------------------------------------------------------------------------------------
# compositing
# ------------------------------------------------------------------------------------------------

COMP_WHITE, COMP_DETACHW = 1, 2


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, z, rows, noise, flags, need_alpha):
        B, S = z.shape
        dev = z.device
        rgb = torch.empty((B, 3), device=dev, dtype=_F32)
        disp = torch.empty((B,), device=dev, dtype=_F32)
        acc = torch.empty_like(disp)
        depth = torch.empty_like(disp)
        weights = torch.empty((B, S), device=dev, dtype=_F32)
        alpha = torch.empty((B, S), device=dev, dtype=_F32) if need_alpha else None
        call('mvip_composite_forward', ptr(raw), ptr(z), ptr(rows), rows.shape[1], ptr(noise), B, S, flags,
             ptr(rgb), ptr(disp), ptr(acc), ptr(depth), ptr(weights), ptr(alpha), stream())
        ctx.save_for_backward(raw, z, rows, noise)
        ctx.flags = flags
        ctx.set_materialize_grads(False)
        if need_alpha:
            return rgb, disp, acc, depth, weights, alpha
        return rgb, disp, acc, depth, weights

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_depth, g_w, g_alpha=None):
        raw, z, rows, noise = ctx.saved_tensors
        B, S = z.shape
        d_raw = torch.empty_like(raw)
        c = lambda g: None if g is None else _f32c(g)
        call('mvip_composite_backward', ptr(raw), ptr(z), ptr(rows), rows.shape[1], ptr(noise), B, S, ctx.flags,
             ptr(c(g_rgb)), ptr(c(g_disp)), ptr(c(g_acc)), ptr(c(g_depth)), ptr(c(g_w)), ptr(c(g_alpha)),
             ptr(d_raw), stream())
        return d_raw, None, None, None, None, None


def composite(raw, z, rows, noise=None, white_bkgd=False, detach_weights=False, need_alpha=False):
    """raw2outputs (DS_NeRF/run_nerf_helpers.py:350-404) -> (rgb, disp, acc, weights, depth, alpha|None).
    `rows` carries the ray direction in columns 3..5; `noise` is already scaled by raw_noise_std."""
    flags = (COMP_WHITE if white_bkgd else 0) | (COMP_DETACHW if detach_weights else 0)
    raw = _f32c(raw)
    z = _f32c(z)
    rows = _f32c(rows)
    noise = None if noise is None else _f32c(noise)
    out = _Composite.apply(raw, z, rows, noise, flags, bool(need_alpha))
    rgb, disp, acc, depth, weights = out[:5]
    return rgb, disp, acc, weights, depth, (out[5] if need_alpha else None)


# ------------------------------------------------------------------------------------------------
# hierarchical sampling
# ------------------------------------------------------------------------------------------------

def sample_pdf_merge(z, weights, u, want_inds=False, want_cdf=False):
    """Fused `sample_pdf(mids, weights[:,1:-1]) -> sort(cat[z, samples])` + z_std
    (DS_NeRF/run.py:1809-1816, :1836).  u: [B,Nf] uniforms, or a 1-D [Nf] row shared by all rays.
    Outputs carry no gradient (the reference detaches z_samples, run.py:1812)."""
    z = _f32c(z.detach())
    w = _f32c(weights.detach())
    u = _f32c(u)
    B, Nc = z.shape
    Nf = u.shape[-1]
    dev = z.device
    zs = torch.empty((B, Nf), device=dev, dtype=_F32)
    zm = torch.empty((B, Nc + Nf), device=dev, dtype=_F32)
    zstd = torch.empty((B,), device=dev, dtype=_F32)
    inds = torch.empty((B, Nf), device=dev, dtype=torch.int64) if want_inds else None
    cdf = torch.empty((B, Nc - 1), device=dev, dtype=_F32) if want_cdf else None
    call('mvip_sample_pdf_merge', ptr(z), ptr(w), ptr(u), int(u.dim() == 1), B, Nc, Nf, ptr(zs), ptr(zm),
         ptr(zstd), ptr(inds, torch.int64), ptr(cdf), stream())
    return zs, zm, zstd, inds, cdf


def sample_pdf(bins, weights, u, want_inds=False, want_cdf=False):
    """Standalone sample_pdf on explicit bins [B,Nb] / weights [B,Nb-1] / uniforms."""
    bins = _f32c(bins)
    w = _f32c(weights)
    u = _f32c(u)
    B, Nb = bins.shape
    Nf = u.shape[-1]
    dev = bins.device
    s = torch.empty((B, Nf), device=dev, dtype=_F32)
    inds = torch.empty((B, Nf), device=dev, dtype=torch.int64) if want_inds else None
    cdf = torch.empty((B, Nb), device=dev, dtype=_F32) if want_cdf else None
    call('mvip_sample_pdf', ptr(bins), ptr(w), ptr(u), int(u.dim() == 1), B, Nb, Nf, ptr(s),
         ptr(inds, torch.int64), ptr(cdf), stream())
    return s, inds, cdf


# ------------------------------------------------------------------------------------------------
# depth -> points -> plane-fit normals
# ------------------------------------------------------------------------------------------------

class _Depth2XYZ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, fx, fy, cx, cy):
        H, W = depth.shape
        pts = torch.empty((H, W, 3), device=depth.device, dtype=_F32)
        call('mvip_depth2xyz', ptr(depth), H, W, fx, fy, cx, cy, ptr(pts), stream())
        ctx.k = (H, W, fx, fy, cx, cy)
        return pts

    @staticmethod
    def backward(ctx, g):
        H, W, fx, fy, cx, cy = ctx.k
        d = torch.empty((H, W), device=g.device, dtype=_F32)
        call('mvip_depth2xyz_backward', ptr(_f32c(g)), H, W, fx, fy, cx, cy, ptr(d), stream())
        return d, None, None, None, None


def depth2xyz(depth, fx, fy, cx, cy):
    """depth [H,W] -> [H,W,3] (DS_NeRF/run.py:1909-1922), differentiable in depth."""
    return _Depth2XYZ.apply(_f32c(depth), float(fx), float(fy), float(cx), float(cy))


class _NormalFit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, k):
        _, H, W = points.shape
        dev = points.device
        moments = torch.empty((9, H, W), device=dev, dtype=_F32)
        scratch = torch.empty((9, H, W), device=dev, dtype=_F32)
        normals = torch.empty((3, H, W), device=dev, dtype=_F32)
        call('mvip_normal_fit_forward', ptr(points), H, W, k, ptr(moments), ptr(scratch), ptr(normals), stream())
        ctx.save_for_backward(points, moments, normals)
        ctx.k = k
        return normals

    @staticmethod
    def backward(ctx, g):
        points, moments, normals = ctx.saved_tensors
        _, H, W = points.shape
        scratch = torch.empty((18, H, W), device=g.device, dtype=_F32)
        d = torch.empty_like(points)
        call('mvip_normal_fit_backward', ptr(points), ptr(moments), ptr(normals), ptr(_f32c(g)), H, W, ctx.k,
             ptr(scratch), ptr(d), stream())
        return d, None


def normal_fit(points, k=31):
    """points [3,H,W] planar -> least-squares plane normals [3,H,W] (DS_NeRF/run.py:1924-1940)."""
    return _NormalFit.apply(_f32c(points), int(k))


# GroupNorm (+ SiLU) of the SDS networks -------------------------------------------------------------

_GN_DTYPES = {torch.float32: 0, torch.float16: 1}


class _ResizeBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, OH, OW):
        xc = _f32c(x)
        N, C, H, W = xc.shape
        y = torch.empty((N, C, OH, OW), device=xc.device, dtype=torch.float32)
        call('mvip_resize_bilinear', ptr(xc), N * C, H, W, OH, OW, ptr(y), stream())
        ctx.shape = (N, C, H, W, OH, OW)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, OH, OW = ctx.shape
        dyc = _f32c(dy)
        dx = torch.empty((N, C, H, W), device=dyc.device, dtype=torch.float32)
        call('mvip_resize_bilinear_backward', ptr(dyc), N * C, H, W, OH, OW, ptr(dx), stream())
        return dx, None, None


def resize_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) for [N, C, H, W] fp32 device tensors (the resize in
    front of vae.encode, DS_NeRF/guidance/sd_utils.py:282-284), differentiable w.r.t. x."""
    return _ResizeBilinear.apply(x, int(size[0]), int(size[1]))


def _gn_workspace(N, C, HW, device):
    nbytes = int(_lib.load().mvip_groupnorm_workspace_bytes(N, C, HW))
    return torch.empty(max(nbytes // 8, 1), device=device, dtype=torch.float64)


class _GroupNorm(torch.autograd.Function):
    """y = act(group_norm(x)) in two HIP launches (csrc/group_norm.hip); dx only: the SDS networks are
    frozen, so a weight or bias that requires grad is an error, not a silent zero."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, silu):
        if x.dtype not in _GN_DTYPES:
            raise _lib.MvipError(f'group_norm: unsupported dtype {x.dtype}')
        if (weight is not None and weight.requires_grad) or (bias is not None and bias.requires_grad):
            raise NotImplementedError('group_norm: parameter gradients are not implemented (frozen networks only)')
        dt = x.dtype
        xc = x.contiguous()
        N, C = xc.shape[0], xc.shape[1]
        HW = xc.numel() // max(N * C, 1)
        w = None if weight is None else weight.detach().to(dt).contiguous()
        b = None if bias is None else bias.detach().to(dt).contiguous()
        y = torch.empty_like(xc)
        mean = torch.empty((N, groups), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        ws = _gn_workspace(N, C, HW, x.device)
        call('mvip_groupnorm_forward', ptr(xc, dt), ptr(w, dt), ptr(b, dt), N, C, HW, int(groups), float(eps),
             int(bool(silu)), _GN_DTYPES[dt], ptr(y, dt), ptr(mean), ptr(rstd), ptr(ws, torch.float64), stream())
        ctx.save_for_backward(xc, w, b, mean, rstd)
        ctx.cfg = (int(groups), int(bool(silu)))
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, w, b, mean, rstd = ctx.saved_tensors
        groups, silu = ctx.cfg
        dt = xc.dtype
        dyc = dy.contiguous().to(dt)
        N, C = xc.shape[0], xc.shape[1]
        HW = xc.numel() // max(N * C, 1)
        dx = torch.empty_like(xc)
        ws = _gn_workspace(N, C, HW, xc.device)
        call('mvip_groupnorm_backward', ptr(xc, dt), ptr(dyc, dt), ptr(w, dt), ptr(b, dt), ptr(mean), ptr(rstd), N, C,
             HW, groups, silu, _GN_DTYPES[dt], ptr(dx, dt), ptr(ws, torch.float64), stream())
        return dx, None, None, None, None, None


def group_norm(x, weight, bias, groups, eps=1e-5, silu=False):
    """act(F.group_norm(x, groups, weight, bias, eps)) for x [N, C, *]; act = SiLU when `silu`."""
    return _GroupNorm.apply(x, weight, bias, groups, eps, silu)


# 3x3 convolution of the SDS networks (split-precision implicit GEMM, csrc/conv3x3.hip) ---------------------

def conv3x3_supported(conv, x, hw=None):
    """True when `conv` (an nn.Conv2d) applied to x [N, Cin, H, W] fp32 can run on the HIP kernel (hw = (H, W) overrides
    x's spatial size: the up-sampled image of Upsample2D, which is never materialised)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if not (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.weight.dtype == torch.float32):
        return False
    lib = _lib.load()
    H, W = (x.shape[2], x.shape[3]) if hw is None else hw
    ok = bool(lib.mvip_conv3x3_supported(conv.out_channels, conv.in_channels, H, W))
    if ok and x.requires_grad and torch.is_grad_enabled():        # the data gradient runs the transposed operator
        ok = bool(lib.mvip_conv3x3_supported(conv.in_channels, conv.out_channels, H, W))
    return ok


# Arithmetic of the SDS networks' contractions (csrc/conv3x3.hip, gemm_f16x3.hip, attention.hip): 0 = split precision (fp16 hi + lo halves of
# both operands, three products: fp32-grade, the fp32 networks), 1 = the reference's --fp16 mode (DS_NeRF/guidance/
# sd_utils.py:66): one fp16 product, hi halves only.  Set for the duration of a network's forward by `precision(...)`
# (guidance/sd_nets.py); autograd Functions remember it for their backward.
PREC = 0


class precision:
    def __init__(self, prec):
        self.prec = int(prec)

    def __enter__(self):
        global PREC
        self.old, PREC = PREC, self.prec

    def __exit__(self, *exc):
        global PREC
        PREC = self.old


def _prec():
    return int(PREC)


# Two products instead of three for weights that are exact fp16 values (prec = 2 of the C ABI; csrc/conv3x3.hip, gemm_f16x3.hip NP = 2).
# The reference always loads `revision="fp16"` weights and, in its default fp32 mode, casts them UP
# (DS_NeRF/guidance/sd_utils.py:69-74): the lo half of every frozen UNet / VAE weight is zero, the third product
# W_lo . x_hi adds exact zeros, and skipping it (and the lo fragments' fetch) changes no bit of any result.  Decided per
# packed image at PACK time (one word read back from the packer: `_note_two_product`); images of anything else -- weights
# with a non-zero lo half, activations packed as an A operand -- keep the three-product kernels.
TWO_PRODUCT = bool(int(_os.environ.get('MVIP_TWO_PRODUCT', '1')))          # A/B switch


def _note_two_product(packed, fragment_bytes):
    """Ask the library whether the packed WEIGHT image's lo fragments are all zero and remember it on the tensor."""
    import ctypes
    flag = ctypes.c_int(0)
    call('mvip_packed_weights_two_product', ptr(packed, torch.uint8), int(fragment_bytes), ctypes.byref(flag), stream())
    packed._mvip_two_product = bool(flag.value)
    return packed


def _prec_w(packed):
    """`prec` for a contraction whose A operand is the packed weight image `packed`."""
    p = _prec()
    return 2 if (p == 0 and TWO_PRODUCT and getattr(packed, '_mvip_two_product', False)) else p


def conv3x3_pack(weight, transpose=False):
    """Packed split-precision image of a [Cout, Cin, 3, 3] weight (transpose: the data-gradient operator)."""
    Cout, Cin = weight.shape[0], weight.shape[1]
    nbytes = int(_lib.load().mvip_conv3x3_packed_bytes(Cout, Cin))
    packed = torch.empty(nbytes, device=weight.device, dtype=torch.uint8)
    w = weight.detach().contiguous()
    call('mvip_conv3x3_pack', ptr(w), Cout, Cin, int(bool(transpose)), ptr(packed, torch.uint8), stream())
    return _note_two_product(packed, Cout * Cin * 36)


def _conv_packed(conv, transpose):
    """Per-module cache of the packed images (the SDS networks are frozen; re-packed if the weight changes)."""
    cache = conv.__dict__.setdefault('_mvip_packed', {})
    key = (conv.weight.data_ptr(), conv.weight._version)
    if cache.get('key') != key:
        cache.clear()
        cache['key'] = key
    if transpose not in cache:
        cache[transpose] = conv3x3_pack(conv.weight, transpose)
    return cache[transpose]


def _split_buffer(N, C, HW, device):
    return torch.empty(N * C * HW * 2, device=device, dtype=torch.float16)


def _with_saved_prec(backward):
    """The backward of an SDS contraction runs in the arithmetic of its forward (ctx.prec), whatever is current."""
    def wrapped(ctx, *grads):
        with precision(getattr(ctx, 'prec', 0)):
            return backward(ctx, *grads)
    return wrapped


def _gn_stats(xc, N, C, H, W, G, eps, ws):
    """mean, rstd [N, G] of xc by a pass over it (fp64 moments, csrc/group_norm.hip)."""
    mean = torch.empty((N, G), device=xc.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call('mvip_groupnorm_stats', ptr(xc), N, C, H * W, G, float(eps), 0, ptr(mean), ptr(rstd), ptr(ws, torch.float64), stream())
    return mean, rstd


class ShortcutLink:
    """Joins the two convolutions of a ResNet block whose shortcut is the identity: the gradient arriving over the shortcut
    (dy of the block) is added to the gradient through the block inside the GroupNorm backward of the FIRST convolution
    (`dx_add` of mvip_groupnorm_backward_fused) instead of by autograd in a pass of its own.  The second convolution's
    backward leaves dy here and reports no gradient for its `residual` input; the first one's picks it up."""
    __slots__ = ('dy',)

    def __init__(self):
        self.dy = None


# The last gradient written by mvip_groupnorm_backward_fused with its per-workgroup maxima: (dx, version, maxima).  The
# backward that receives exactly this tensor as its dy takes the scale from the maxima instead of re-reading it.  The
# strong reference keeps the memory from being reused under the same address; one entry, dropped at the next lookup.
_LAST_DX = [None]


def _scale_of_gradient(dyc):
    """scale2 of dyc: from the maxima its producer left (same power of two) or by the absmax pass."""
    dev = dyc.device
    scale2 = torch.empty(4, device=dev, dtype=torch.float32)
    last, _LAST_DX[0] = _LAST_DX[0], None
    if (last is not None and last[0].data_ptr() == dyc.data_ptr() and last[0].numel() == dyc.numel()
            and last[0]._version == last[1] and dyc._version == last[1] and dyc.dtype == torch.float32):
        call('mvip_absmax_scale_from_maxima', ptr(last[2]), last[2].numel(), ptr(scale2), stream())
    else:
        call('mvip_absmax_scale', ptr(dyc), dyc.numel(), ptr(scale2), ptr(_zero_words(dev)[32:34], torch.int32), stream())
    return scale2


class _NormActConv3x3(torch.autograd.Function):
    """conv3x3(act(group_norm(x))) + bias [+ chan_add[:, :, None, None]] [+ residual]: statistics, split-plane
    writer (normalise + SiLU fused) and the MFMA convolution.  Backward: dY -> split planes (scaled by a power of
    two from its absolute maximum) -> the same kernel with the transposed weight image -> GroupNorm backward.
    Parameter gradients are not produced (frozen networks)."""

    @staticmethod
    def forward(ctx, x, chan_add, residual, norm, conv, silu, link=None):
        ctx.prec = _prec()
        for p in (norm.weight, norm.bias, conv.weight, conv.bias):
            if p is not None and p.requires_grad:
                raise NotImplementedError('conv3x3: parameter gradients are not implemented (frozen networks only)')
        xc = x.contiguous()
        N, C, H, W = xc.shape
        HW, G, Cout = H * W, norm.num_groups, conv.out_channels
        dev = xc.device
        ws = _gn_workspace(N, C, HW, dev)
        gw = None if norm.weight is None else norm.weight.detach().contiguous()
        gb = None if norm.bias is None else norm.bias.detach().contiguous()
        xs = _split_buffer(N, C, HW, dev)
        keep_stats = ctx.needs_input_grad[0] or C // G < 4
        if keep_stats and C // G >= 4 and STATS_FROM_PLANE_WRITER:
            # the backward needs mean / rstd: the plane writer reduces the moment partials (as below) AND writes them out --
            # the same bits gn_finalize would write, without its launch
            rm = _row_moments_of(xc)
            if rm is None:
                call('mvip_groupnorm_stats', ptr(xc), N, C, HW, G, float(norm.eps), 0, None, None, ptr(ws, torch.float64), stream())
                rm = ws
            mean = torch.empty((N, G), device=dev, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            call('mvip_groupnorm_split_planes_moments_out', ptr(xc), ptr(gw), ptr(gb), ptr(rm, torch.float64), float(norm.eps),
                 N, C, HW, G, int(bool(silu)), ptr(xs, torch.float16), ptr(mean), ptr(rstd), _prec(), stream())
            ctx.save_for_backward(xc, gw, gb, mean, rstd)
        elif keep_stats:
            mean, rstd = _gn_stats(xc, N, C, H, W, G, norm.eps, ws)
            call('mvip_groupnorm_split_planes', ptr(xc), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N, C, HW, G,
                 int(bool(silu)), ptr(xs, torch.float16), _prec(), stream())
            ctx.save_for_backward(xc, gw, gb, mean, rstd)
        else:       # nobody needs mean / rstd afterwards: the plane writer reduces the moment partials itself (one launch less)
            rm = _row_moments_of(xc)                  # ... and the producing convolution may have left them already
            if rm is None:
                call('mvip_groupnorm_stats', ptr(xc), N, C, HW, G, float(norm.eps), 0, None, None, ptr(ws, torch.float64), stream())
                rm = ws
            call('mvip_groupnorm_split_planes_moments', ptr(xc), ptr(gw), ptr(gb), ptr(rm, torch.float64), float(norm.eps),
                 N, C, HW, G, int(bool(silu)), ptr(xs, torch.float16), _prec(), stream())
        y = torch.empty((N, Cout, H, W), device=dev, dtype=torch.float32)
        bias = None if conv.bias is None else conv.bias.detach().contiguous()
        ca = None if chan_add is None else chan_add.detach().contiguous()
        rs = None if residual is None else residual.detach().contiguous()
        _conv3x3_launch(xs, _conv_packed(conv, False), bias, ca, rs, None, N, C, Cout, H, W, y, moments=True)
        ctx.mods = (norm, conv, bool(silu))
        ctx.link = link
        ctx.link_tail = link is not None and residual is not None      # the block's second convolution
        return y

    @staticmethod
    @_with_saved_prec
    def backward(ctx, dy):
        norm, conv, silu = ctx.mods
        dyc = dy.contiguous().float()
        dx = None
        link = ctx.link
        if ctx.needs_input_grad[0]:
            xc, gw, gb, mean, rstd = ctx.saved_tensors
            N, C, H, W = xc.shape
            HW, Cout, dev = H * W, conv.out_channels, xc.device
            if not _lib.load().mvip_conv3x3_supported(C, Cout, H, W):
                raise NotImplementedError(f'conv3x3 data gradient: unsupported shape Cin={C} Cout={Cout}')
            scale2 = _scale_of_gradient(dyc)
            dys = _split_buffer(N, Cout, HW, dev)
            call('mvip_split_planes', ptr(dyc), N, Cout, HW, ptr(scale2), ptr(dys, torch.float16), _prec(), stream())
            dact = torch.empty_like(xc)
            _conv3x3_launch(dys, _conv_packed(conv, True), None, None, None, scale2, N, Cout, C, H, W, dact)
            del dys
            dx = torch.empty_like(xc)
            ws = _gn_workspace(N, C, HW, dev)
            add = None
            if link is not None and not ctx.link_tail:           # first convolution of a linked block: + the shortcut's gradient
                add, link.dy = link.dy, None
            maxima = torch.empty(int(_lib.load().mvip_groupnorm_backward_maxima(N, C, HW)), device=dev, dtype=torch.float32)
            call('mvip_groupnorm_backward_fused', ptr(xc), ptr(dact), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N, C, HW,
                 norm.num_groups, int(silu), 0, ptr(add), ptr(dx), ptr(maxima), ptr(ws, torch.float64), stream())
            _LAST_DX[0] = (dx, dx._version, maxima)
        d_ca = dyc.sum((2, 3)) if ctx.needs_input_grad[1] else None
        d_rs = dyc if ctx.needs_input_grad[2] else None
        if ctx.link_tail and d_rs is not None:
            link.dy, d_rs = dyc, None                            # handed to the first convolution's GroupNorm backward
        return dx, d_ca, d_rs, None, None, None, None


# The last convolution output whose channel-split reduction also left its GroupNorm row moments: (y, version, moments).
# A forward-only GroupNorm that is handed exactly this tensor skips its pass over y (mvip_groupnorm_split_planes_moments
# reads the moments directly).  One entry; the strong reference keeps the address from being reused.
_LAST_Y = [None]
ROW_MOMENTS = True             # A/B switch: False = every GroupNorm computes its moments from its input
TILE_MOMENTS = _os.environ.get('MVIP_TILE_MOMENTS', '1') != '0'   # A/B switch: unsplit convolutions leave moment partials too (round 6)
STATS_FROM_PLANE_WRITER = True # A/B switch: False = mean / rstd of a forward with grad come from gn_finalize (one launch more)


def _row_moments_of(xc):
    last, _LAST_Y[0] = _LAST_Y[0], None
    if (last is not None and last[0].data_ptr() == xc.data_ptr() and last[0].shape == xc.shape and xc.dtype == torch.float32
            and xc._version == last[1] and last[0]._version == last[1]):
        return last[2]
    return None


def _conv3x3_launch(xs, packed, bias, chan_add, residual, scale2, N, Cin, Cout, H, W, y, moments=False):
    """mvip_conv3x3_f16x3_ws with the split-K workspace the library asks for this shape (none for most).  moments: a
    channel-split launch also leaves y's GroupNorm row moments for the next layer (registered in _LAST_Y)."""
    nbytes = int(_lib.load().mvip_conv3x3_workspace_bytes(N, Cin, Cout, H, W))
    ws = torch.empty(nbytes // 4, device=y.device, dtype=torch.float32) if nbytes else None
    if moments and ROW_MOMENTS and nbytes:
        nd = int(_lib.load().mvip_conv3x3_row_moments_doubles(N, Cin, Cout, H, W))
        if nd:
            rm = torch.empty(nd, device=y.device, dtype=torch.float64)
            call('mvip_conv3x3_f16x3_ws_moments', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add),
                 ptr(residual), ptr(scale2), N, Cin, Cout, H, W, ptr(y), ptr(ws), ptr(rm, torch.float64), _prec_w(packed), stream())
            _LAST_Y[0] = (y, y._version, rm)
            return
    if moments and ROW_MOMENTS and TILE_MOMENTS and not nbytes:
        # an unsplit launch: moment partials per (pixel tile, wave) from the epilogue + a small reduction (round 6), instead of
        # the next GroupNorm's pass over y
        sb = int(_lib.load().mvip_conv3x3_tile_moments_scratch_bytes(N, Cin, Cout, H, W))
        if sb:
            tp = torch.empty(sb // 4, device=y.device, dtype=torch.float32)
            rm = torch.empty(int(_lib.load().mvip_groupnorm_workspace_bytes(N, Cout, H * W)) // 8, device=y.device, dtype=torch.float64)
            call('mvip_conv3x3_f16x3_tile_moments', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add),
                 ptr(residual), ptr(scale2), N, Cin, Cout, H, W, ptr(y), ptr(tp), ptr(rm, torch.float64), _prec_w(packed), stream())
            _LAST_Y[0] = (y, y._version, rm)
            return
    call('mvip_conv3x3_f16x3_ws', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add),
         ptr(residual), ptr(scale2), N, Cin, Cout, H, W, ptr(y), ptr(ws), _prec_w(packed), stream())


def conv3x3_plain(x, conv, upsample2=False):
    """conv(x) (+ bias) for a 3x3 / stride 1 / padding 1 convolution on the split-precision MFMA kernel, without a
    preceding GroupNorm and without autograd: the UNet's up-sampling convolutions (the UNet runs under no_grad).  The
    input is scaled by a power of two from its absmax before the fp16 hi/lo split, as the data gradient is.
    upsample2: the convolution runs on the 2x nearest-neighbour up-sampled image, which is never materialised (the plane
    writer reads x[oy / 2][ox / 2]; the absolute maximum is that of x itself)."""
    xc = _f32c(x.detach())
    N, C, H, W = xc.shape
    Cout, dev = conv.out_channels, xc.device
    scale2 = unit_scale(dev) if forward_unit_scale() else absmax_scale(xc)
    if upsample2:
        xs = _split_buffer(N, C, 4 * H * W, dev)
        call('mvip_split_planes_upsample2', ptr(xc), N, C, H, W, ptr(scale2), ptr(xs, torch.float16), _prec(), stream())
        H, W = 2 * H, 2 * W
    else:
        xs = _split_buffer(N, C, H * W, dev)
        call('mvip_split_planes', ptr(xc), N, C, H * W, ptr(scale2), ptr(xs, torch.float16), _prec(), stream())
    y = torch.empty((N, Cout, H, W), device=dev, dtype=torch.float32)
    bias = None if conv.bias is None else _f32c(conv.bias.detach())
    _conv3x3_launch(xs, _conv_packed(conv, False), bias, None, None, scale2, N, C, Cout, H, W, y)
    return y


def norm_act_conv3x3(x, norm, conv, silu=True, chan_add=None, residual=None, link=None):
    """conv(act(norm(x))) [+ chan_add[:, :, None, None]] [+ residual] on the HIP kernels; the caller checks
    conv3x3_supported first.  link: a ShortcutLink shared by the two convolutions of an identity-shortcut block."""
    return _NormActConv3x3.apply(x, chan_add, residual, norm, conv, silu, link)


# Hash-grid model (NeRF_TCNN) -----------------------------------------------------------------------------

class _HashGrid(torch.autograd.Function):
    """Multiresolution hash-grid features [32, P] (level-major) of points x [P, 3]; gradient w.r.t. the table
    by fp32 atomics (positions never need a gradient on this path).  half2=True: the scattered fine-level
    contributions go out as half-precision pair atomics (tiny-cuda-nn's arithmetic; half the atomic count)."""

    @staticmethod
    def forward(ctx, x, table, levels, bound, half2):
        xc = _f32c(x.detach())
        tc = table.detach().contiguous()
        P = xc.shape[0]
        out = torch.empty((32, P), device=xc.device, dtype=torch.float32)
        call('mvip_hashgrid_forward', ptr(xc), ptr(tc), ptr(levels, torch.int32), P, float(bound), ptr(out), stream())
        ctx.save_for_backward(xc, levels)
        ctx.meta = (float(bound), tc.numel(), bool(half2))
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, levels = ctx.saved_tensors
        bound, n, half2 = ctx.meta
        d = dout.contiguous().float()
        dtable = torch.zeros(n, device=xc.device, dtype=torch.float32)
        if half2:
            scale2 = absmax_scale(d)
            dtable_h = torch.zeros(n, device=xc.device, dtype=torch.float16)
            call('mvip_hashgrid_backward_half2', ptr(xc), ptr(d), ptr(levels, torch.int32), xc.shape[0], bound,
                 ptr(scale2), ptr(dtable), ptr(dtable_h, torch.float16), stream())
            dtable += dtable_h.float() * (16.0 * scale2[1])
        else:
            call('mvip_hashgrid_backward', ptr(xc), ptr(d), ptr(levels, torch.int32), xc.shape[0], bound, ptr(dtable),
                 stream())
        return None, dtable, None, None, None


def hashgrid_encode(x, table, levels, bound=0.0, half2_atomics=False):
    """x [P,3] (raw coordinates in [-bound, bound], or already in [0,1] when bound == 0), table flat
    [n_entries*2], levels [16,4] int32 -> [32, P]."""
    return _HashGrid.apply(x, table, levels, bound, half2_atomics)


def sh4(dirs):
    """Degree-4 spherical harmonics [16, P] of unit directions [P, 3] (NeRF_TCNN's input convention)."""
    dc = _f32c(dirs.detach())
    out = torch.empty((16, dc.shape[0]), device=dc.device, dtype=torch.float32)
    call('mvip_sh4', ptr(dc), dc.shape[0], ptr(out), stream())
    return out


def hashgrid_mlp_pack(sigma_params, colour_params):
    """Operand image of NeRF_TCNN's five bias-free matrices for `hashgrid_nerf_forward`."""
    sp, cp = _f32c(sigma_params.detach()), _f32c(colour_params.detach())
    assert sp.numel() == 3072 and cp.numel() == 7168
    img = torch.empty(int(_lib.load().mvip_hashgrid_mlp_packed_floats()), device=sp.device, dtype=torch.float32)
    call('mvip_hashgrid_mlp_pack', ptr(sp), ptr(cp), ptr(img), stream())
    return img


def hashgrid_nerf_forward(x, dirs, table, levels, img, bound):
    """Fused no-grad NeRF_TCNN.forward: x [P,3], dirs [P,3] -> [P,4] = (colour, sigma)."""
    xc, dc = _f32c(x.detach()), _f32c(dirs.detach())
    P = xc.shape[0]
    out = torch.empty((P, 4), device=xc.device, dtype=torch.float32)
    call('mvip_hashgrid_nerf_forward', ptr(xc), ptr(dc), ptr(table.detach().contiguous()), ptr(levels, torch.int32),
         ptr(img), P, float(bound), ptr(out), stream())
    return out


def skinny_wgrad(dY, X):
    """dW [M, N] = dY [M, P] @ X [N, P]^T for the hash-grid model's small layers (M, N <= 64, P % 64 == 0)."""
    dYc, Xc = _f32c(dY), _f32c(X)
    M, P = dYc.shape
    N = Xc.shape[0]
    slabs = torch.empty((int(_lib.load().mvip_skinny_wgrad_slabs(P)), M, N), device=dYc.device, dtype=torch.float32)
    call('mvip_skinny_wgrad', ptr(dYc), ptr(Xc), M, N, P, ptr(slabs), stream())
    return slabs.sum(0)


# Forward / data gradient of the hash-grid model's small layers run on skinny_fwd_kernel / skinny_fwd16_kernel (default since
# round 4; MVIP_SKINNY_LINEAR=0 puts torch matmuls back for these two products as the A/B alternative; the weight gradient
# is skinny_wgrad_kernel either way).  Measured on the training iteration
# (tools/hashgrid_train_profile.py, same box, alternating) in round 3 with 32-row tiles only: 15.6 ms with the kernel, 15.2 ms
# with the library, whose 16-row MFMA tiles did half the matrix work on the 16-row layers -- those layers now have a 16-row
# kernel of their own.
SKINNY_LINEAR = bool(int(_os.environ.get('MVIP_SKINNY_LINEAR', '1')))


def _skinny_ok(W, X):
    return (SKINNY_LINEAR and X.is_cuda and X.dtype == torch.float32 and W.dtype == torch.float32 and W.shape[0] <= 64 and W.shape[1] <= 64
            and X.shape[1] > 0)


def _pad_points(X, multiple):
    """X [C, P] with P rounded up to `multiple` by zero columns (ragged last chunks only: the kernels read 16-byte quads)."""
    pad = (-X.shape[1]) % multiple
    return X if pad == 0 else torch.nn.functional.pad(X, (0, pad))


def skinny_linear(W, X, relu=False, transpose=False):
    """act(W X) (or act(W^T X) with transpose) for the hash-grid model's small layers: X [N, P] channel-major,
    csrc/skinny_gemm.hip::skinny_fwd_kernel / skinny_fwd16_kernel (exact fp32, one streaming pass)."""
    Wc = _f32c(W)
    P0 = X.shape[1]
    Xc = _f32c(_pad_points(X, 4))
    M, N = (Wc.shape[1], Wc.shape[0]) if transpose else (Wc.shape[0], Wc.shape[1])
    P = Xc.shape[1]
    Y = torch.empty((M, P), device=Xc.device, dtype=torch.float32)
    sm, sn = (1, Wc.shape[1]) if transpose else (Wc.shape[1], 1)
    call('mvip_skinny_linear', ptr(Wc), sm, sn, ptr(Xc), M, N, P, int(bool(relu)), ptr(Y), stream())
    return Y if P == P0 else Y[:, :P0].contiguous()


class _LinearCM(torch.autograd.Function):
    """Y [M, P] = act(W [M, N] @ X [N, P]) (channel-major activations, act = ReLU or identity).  Forward and data gradient:
    csrc/skinny_gemm.hip::skinny_fwd_kernel (16-row variant for M <= 16); the weight gradient -- a [M, N] result contracted
    over millions of points, which a BLAS library runs on a handful of workgroups -- is skinny_wgrad_kernel.  Library
    matmuls only for layers wider than 64 (none in NeRF_TCNN) or with MVIP_SKINNY_LINEAR=0."""

    @staticmethod
    def forward(ctx, W, X, relu):
        if _skinny_ok(W, X):
            Y = skinny_linear(W, X, relu)
        else:
            Y = W @ X
            if relu:
                Y = torch.relu(Y)
        ctx.save_for_backward(W, X, Y if relu else None)
        ctx.relu = relu
        return Y

    @staticmethod
    def backward(ctx, dY):
        W, X, Y = ctx.saved_tensors
        dZ = dY * (Y > 0) if ctx.relu else dY
        dW = dX = None
        if ctx.needs_input_grad[1]:
            dX = skinny_linear(W, dZ, False, transpose=True) if _skinny_ok(W.t(), dZ) else W.t() @ dZ
        if ctx.needs_input_grad[0]:
            if X.is_cuda and X.dtype == torch.float32 and W.shape[0] <= 64 and W.shape[1] <= 64 and X.shape[1] > 0:
                dW = skinny_wgrad(_pad_points(dZ, 64), _pad_points(X, 64))      # zero columns add nothing
            else:
                dW = dZ @ X.t()
        return dW, dX, None


def linear_cm(W, X, relu=False):
    return _LinearCM.apply(W, X, bool(relu))


# Split-precision GEMM building blocks (csrc/f16x3_producers.hip, csrc/gemm_f16x3.hip) and the VAE mid-block attention built from them ---

ABSMAX_THREE_LAUNCHES = bool(int(_os.environ.get('MVIP_ABSMAX_THREE_LAUNCHES', '0')))     # A/B switch: zero + reduce + scale


def absmax_scale(t):
    """Device-side {s, 1/s, scratch, scratch}: power of two with |t|max * s in [2^9, 2^10)."""
    tc = t.contiguous()
    scale2 = torch.empty(4, device=t.device, dtype=torch.float32)
    zw = None if ABSMAX_THREE_LAUNCHES else _zero_words(t.device)[32:34]
    call('mvip_absmax_scale', ptr(tc), tc.numel(), ptr(scale2), ptr(zw, torch.int32), stream())
    return scale2


def gemm_pack_a(src, M, K, sm, sk, weights=False):
    """A[m][k] = src.flatten()[m*sm + k*sk] (src a dense block of M*K floats) -> packed split-precision image.
    weights=True: a frozen layer's weights, packed once -- the packer's "lo fragments are zero" word is read back (a host
    synchronisation, which is why activations packed per step never ask) so that its contractions can run two products."""
    s = src.contiguous()
    assert s.numel() == M * K
    packed = torch.empty(int(_lib.load().mvip_gemm_packed_bytes(M, K)), device=s.device, dtype=torch.uint8)
    call('mvip_gemm_pack_a', ptr(s), M, K, sm, sk, ptr(packed, torch.uint8), stream())
    return _note_two_product(packed, M * K * 4) if weights else packed


def split_planes_strided(x, N, K, P, sn, sc, sp, scale2=None):
    """X[n][k][p] = x.flatten()[n*sn + k*sc + p*sp] (* scale2[0]) -> fp16 hi/lo split planes."""
    xc = x.contiguous()
    xs = _split_buffer(N, K, P, xc.device)
    call('mvip_split_planes_strided', ptr(xc), N, K, P, sn, sc, sp, ptr(scale2), ptr(xs, torch.float16), _prec(), stream())
    return xs


GEMM_CFG = 0       # 0: tile chosen by shape; 1..4 force a workgroup tile (A/B timing switch, see include/mvip_nerf.h)


LN_STATS_FROM_GEMM = True      # A/B switch: False = every LayerNorm computes its statistics from its input (one launch more)


def gemm_f16x3(xs, packed, N, K, M, P, bias=None, chan_add=None, residual=None, x_scale2=None, out=None, ln_stats=False):
    """Y[n][m][p] = sum_k A[m][k] X[n][k][p] (+ bias[m] + chan_add[n][m] + residual[n][m][p]), fp32 [N, M, P].
    out: a contiguous fp32 tensor of N * M * P elements to write instead of a new one (e.g. a slice of a larger result).
    ln_stats: returns (Y, stats) -- stats = (fp64 partial moments of Y over its rows, segments) for `layernorm_split(...,
    stats=)` when this shape's launch can leave them in its epilogue (round 6), else None."""
    if out is not None:
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == N * M * P
        y = out
    else:
        y = torch.empty((N, M, P), device=xs.device, dtype=torch.float32)
    if GEMM_CFG:
        call('mvip_gemm_f16x3_cfg', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add),
             ptr(residual), ptr(x_scale2), N, K, M, P, ptr(y), int(GEMM_CFG), _prec_w(packed), stream())
        return (y, None) if ln_stats else y
    nbytes = int(_lib.load().mvip_gemm_workspace_bytes(N, K, M, P))            # split-K partial sums (few shapes)
    ws = torch.empty(nbytes // 4, device=y.device, dtype=torch.float32) if nbytes else None
    if ln_stats:
        S = int(_lib.load().mvip_gemm_ln_segments(N, K, M, P, _prec_w(packed))) if (LN_STATS_FROM_GEMM and not GEMM_CFG) else 0
        if S:
            part = torch.empty(N * S * 2 * P, device=y.device, dtype=torch.float64)
            call('mvip_gemm_f16x3_ws_ln', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add), ptr(residual),
                 ptr(x_scale2), N, K, M, P, ptr(y), ptr(ws), ptr(part, torch.float64), _prec_w(packed), stream())
            return y, (part, S)
    call('mvip_gemm_f16x3_ws', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(chan_add), ptr(residual),
         ptr(x_scale2), N, K, M, P, ptr(y), ptr(ws), _prec_w(packed), stream())
    return (y, None) if ln_stats else y


# Opt-in: split the forward ACTIVATIONS of the UNet (evaluated under no_grad) at a fixed scale of 1 instead of a
# measured power of two.  They live well inside fp16's range (the reference's own --fp16 mode runs the whole UNet in
# fp16, DS_NeRF/guidance/sd_utils.py:66), and every absmax pass disappears from the step -- but the result is then
# fp32-grade only relative to a tensor scale of O(0.1 .. 1e4): for a tensor of magnitude 1e-4 the fp16 lo terms are
# subnormal and the error grows to fp16-grade (tests/test_sds.py::test_plain_conv3x3_on_mfma_kernel shows it).  The
# default keeps the measured scale, which is magnitude-invariant.
FORWARD_UNIT_SCALE = False         # opt-in (34.5 vs 35.x ms per SDS step): see the comment above for what it gives up
_UNIT = {}


_PROB = {}


def prob_scale(device):
    """scale2 = {2^9, 2^-9} for softmax probabilities (values in [0, 1]: the bound IS the scale, no pass over the [L, L] matrix
    for its maximum; a flat row's 1/L = 2^-12 still splits into normal fp16 hi + lo terms at this scale)."""
    if device not in _PROB:
        _PROB[device] = torch.tensor([512.0, 1.0 / 512.0, 0.0, 0.0], device=device, dtype=_F32)
    return _PROB[device]


def unit_scale(device):
    if device not in _UNIT:
        _UNIT[device] = torch.tensor([1.0, 1.0, 0.0, 0.0], device=device, dtype=_F32)
    return _UNIT[device]


def forward_unit_scale():
    """True when FORWARD activations are split at scale 1: the opt-in above, and always in the reference's --fp16 mode
    (PREC = 1) -- there the single hi plane fp16(x) IS the fp16 tensor the reference's half-precision networks hold
    (DS_NeRF/guidance/sd_utils.py:66), so a measured scale would buy nothing the mode promises.  Gradients keep their
    measured scale in both modes (they are ~1e-5 and would underflow)."""
    return FORWARD_UNIT_SCALE or _prec() == 1


def _scaled_planes(x, N, K, P, sn, sc, sp, forward_activation=False):
    s2 = unit_scale(x.device) if (forward_activation and forward_unit_scale()) else absmax_scale(x)
    return split_planes_strided(x, N, K, P, sn, sc, sp, s2), s2


def vae_attention_supported(x):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] % 32 == 0
            and (x.shape[2] * x.shape[3]) % 256 == 0)


def _attn_weights(mod):
    """Cached packed images of the attention block's four linears (frozen): [Wq;Wk;Wv] and Wo with their
    transposes for the backward."""
    ws = (mod.to_q.weight, mod.to_k.weight, mod.to_v.weight, mod.to_out[0].weight)
    key = tuple((w.data_ptr(), w._version) for w in ws)
    cache = mod.__dict__.setdefault('_mvip_packed', {})
    if cache.get('key') != key:
        C = ws[0].shape[0]
        wqkv = torch.cat([w.detach() for w in ws[:3]], 0).contiguous()          # [3C, C]
        wo = ws[3].detach().contiguous()
        cache.clear()
        cache.update(key=key,
                     qkv=gemm_pack_a(wqkv, 3 * C, C, C, 1, weights=True), qkv_t=gemm_pack_a(wqkv, C, 3 * C, 1, C, weights=True),
                     o=gemm_pack_a(wo, C, C, C, 1, weights=True), o_t=gemm_pack_a(wo, C, C, 1, C, weights=True),
                     bqkv=torch.cat([mod.to_q.bias.detach(), mod.to_k.bias.detach(), mod.to_v.bias.detach()]).contiguous(),
                     bo=mod.to_out[0].bias.detach().contiguous())
    return cache


class _VAEAttention(torch.autograd.Function):
    """x + proj(softmax(q^T k / sqrt(C)) v) of the VAE mid block (single head over H*W tokens, channel-first),
    every product on the split-precision MFMA GEMM; the [L, L] score matrix is materialised (67 MB at 64x64).
    Backward: the six transposed products + GroupNorm backward.  Parameter gradients are not produced."""

    @staticmethod
    def forward(ctx, x, mod):
        ctx.prec = _prec()
        for p in mod.parameters():
            if p.requires_grad:
                raise NotImplementedError('vae_attention: parameter gradients are not implemented (frozen networks only)')
        xc = x.contiguous()
        N, C, H, W = xc.shape
        L, dev, norm = H * W, xc.device, mod.group_norm
        G = norm.num_groups
        wts = _attn_weights(mod)
        ws = _gn_workspace(N, C, L, dev)
        gw, gb = norm.weight.detach().contiguous(), norm.bias.detach().contiguous()
        mean, rstd = _gn_stats(xc, N, C, H, W, G, norm.eps, ws)
        hs = _split_buffer(N, C, L, dev)
        call('mvip_groupnorm_split_planes', ptr(xc), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N, C, L, G, 0,
             ptr(hs, torch.float16), _prec(), stream())
        qkv = gemm_f16x3(hs, wts['qkv'], N, C, 3 * C, L, bias=wts['bqkv'])           # [N, 3C, L]
        del hs
        probs, O = [], torch.empty((N, C, L), device=dev, dtype=torch.float32)
        for n in range(N):
            q, k, v = qkv[n, :C], qkv[n, C:2 * C], qkv[n, 2 * C:]
            ks, s2 = _scaled_planes(k, 1, C, L, 0, L, 1, forward_activation=_prec() == 1)
            S = gemm_f16x3(ks, gemm_pack_a(q, L, C, 1, L), 1, C, L, L, x_scale2=s2)[0]        # S[i][j] = q_i . k_j
            Pm = softmax_rows(S, C ** -0.5)
            del S
            s2 = unit_scale(dev) if _prec() == 1 else prob_scale(dev)
            pts = split_planes_strided(Pm, 1, L, L, 0, 1, L, s2)                              # X[k=j][p=i] = P[i][j]
            gemm_f16x3(pts, gemm_pack_a(v, C, L, L, 1), 1, L, C, L, x_scale2=s2, out=O[n])
            probs.append(Pm)
        os_, s2 = _scaled_planes(O, N, C, L, C * L, L, 1, forward_activation=_prec() == 1)
        out = gemm_f16x3(os_, wts['o'], N, C, C, L, bias=wts['bo'], residual=xc.reshape(N, C, L), x_scale2=s2)
        ctx.save_for_backward(xc, gw, gb, mean, rstd, qkv, *probs)
        ctx.mod = mod
        return out.reshape(N, C, H, W)

    @staticmethod
    @_with_saved_prec
    def backward(ctx, dout):
        xc, gw, gb, mean, rstd, qkv, *probs = ctx.saved_tensors
        mod = ctx.mod
        N, C, H, W = xc.shape
        L, dev, norm = H * W, xc.device, mod.group_norm
        wts = _attn_weights(mod)
        d = dout.contiguous().float().reshape(N, C, L)
        ds, s2 = _scaled_planes(d, N, C, L, C * L, L, 1)
        dO = gemm_f16x3(ds, wts['o_t'], N, C, C, L, x_scale2=s2)                               # Wo^T dOut
        dqkv = torch.empty_like(qkv)
        for n in range(N):
            q, k, v, Pm = qkv[n, :C], qkv[n, C:2 * C], qkv[n, 2 * C:], probs[n]
            s2 = prob_scale(dev)
            ps = split_planes_strided(Pm, 1, L, L, 0, L, 1, s2)                                # X[k=i][p=j] = P[i][j]
            gemm_f16x3(ps, gemm_pack_a(dO[n], C, L, L, 1), 1, L, C, L, x_scale2=s2, out=dqkv[n, 2 * C:])        # dV
            vs, s2 = _scaled_planes(v, 1, C, L, 0, L, 1)
            dP = gemm_f16x3(vs, gemm_pack_a(dO[n], L, C, 1, L), 1, C, L, L, x_scale2=s2)[0]    # dP[i][j] = dO_i . v_j
            dS = softmax_rows_backward(Pm, dP, C ** -0.5)
            del dP
            s2 = absmax_scale(dS)
            dst = split_planes_strided(dS, 1, L, L, 0, 1, L, s2)                               # X[k=j][p=i] = dS[i][j]
            gemm_f16x3(dst, gemm_pack_a(k, C, L, L, 1), 1, L, C, L, x_scale2=s2, out=dqkv[n, :C])               # dQ
            dsn = split_planes_strided(dS, 1, L, L, 0, L, 1, s2)                               # X[k=i][p=j] = dS[i][j]
            gemm_f16x3(dsn, gemm_pack_a(q, C, L, L, 1), 1, L, C, L, x_scale2=s2, out=dqkv[n, C:2 * C])          # dK
        dqs, s2 = _scaled_planes(dqkv, N, 3 * C, L, 3 * C * L, L, 1)
        dh = gemm_f16x3(dqs, wts['qkv_t'], N, 3 * C, C, L, x_scale2=s2)                         # Wqkv^T dqkv
        dx = torch.empty_like(xc)
        ws = _gn_workspace(N, C, L, dev)
        # + the gradient arriving over the block's residual connection, and the maxima of the sum for the next backward's scale
        maxima = torch.empty(int(_lib.load().mvip_groupnorm_backward_maxima(N, C, L)), device=dev, dtype=torch.float32)
        call('mvip_groupnorm_backward_fused', ptr(xc), ptr(dh.reshape(N, C, H, W)), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N,
             C, L, norm.num_groups, 0, 0, ptr(d), ptr(dx), ptr(maxima), ptr(ws, torch.float64), stream())
        _LAST_DX[0] = (dx, dx._version, maxima)
        return dx, None


def vae_attention(x, mod):
    return _VAEAttention.apply(x, mod)


# 1x1 convolutions of the SDS networks on the split-precision GEMM (csrc/gemm_f16x3.hip) ---------------------------

def conv1x1_supported(conv, x, tokens=False):
    """x: [N, Cin, H, W] (or [N, L, Cin] token-major when tokens=True), fp32 on the device."""
    if not (x.is_cuda and x.dtype == torch.float32 and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.weight.dtype == torch.float32):
        return False
    L = x.shape[1] if tokens else x.shape[2] * x.shape[3]
    return conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0 and L % 256 == 0


def _conv1x1_packed(conv, transpose):
    cache = conv.__dict__.setdefault('_mvip_packed', {})
    key = (conv.weight.data_ptr(), conv.weight._version)
    if cache.get('key') != key:
        cache.clear()
        cache['key'] = key
    if transpose not in cache:
        Cout, Cin = conv.out_channels, conv.in_channels
        w = conv.weight.detach().reshape(Cout, Cin).contiguous()
        cache[transpose] = gemm_pack_a(w, Cin, Cout, 1, Cin, weights=True) if transpose else gemm_pack_a(w, Cout, Cin, Cin, 1, weights=True)
    return cache[transpose]


class _Conv1x1(torch.autograd.Function):
    """conv1x1(x) + bias [+ residual] for x [N, Cin, H, W]; the data gradient runs the transposed image."""

    @staticmethod
    def forward(ctx, x, residual, conv):
        ctx.prec = _prec()
        if conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad):
            raise NotImplementedError('conv1x1: parameter gradients are not implemented (frozen networks only)')
        xc = x.contiguous()
        N, C, H, W = xc.shape
        L, Cout = H * W, conv.out_channels
        xs, s2 = _scaled_planes(xc, N, C, L, C * L, L, 1, forward_activation=(not x.requires_grad) or _prec() == 1)
        bias = None if conv.bias is None else conv.bias.detach().contiguous()
        rs = None if residual is None else residual.detach().contiguous()
        y = gemm_f16x3(xs, _conv1x1_packed(conv, False), N, C, Cout, L, bias=bias, residual=rs, x_scale2=s2)
        ctx.conv, ctx.shape = conv, (N, C, H, W)
        return y.reshape(N, Cout, H, W)

    @staticmethod
    @_with_saved_prec
    def backward(ctx, dy):
        conv = ctx.conv
        N, C, H, W = ctx.shape
        L, Cout = H * W, conv.out_channels
        d = dy.contiguous().float()
        dx = None
        if ctx.needs_input_grad[0]:
            ds, s2 = _scaled_planes(d, N, Cout, L, Cout * L, L, 1)
            dx = gemm_f16x3(ds, _conv1x1_packed(conv, True), N, Cout, C, L, x_scale2=s2).reshape(N, C, H, W)
        return dx, (d if ctx.needs_input_grad[1] else None), None


def conv1x1(x, conv, residual=None):
    return _Conv1x1.apply(x, residual, conv)


# General convolution as im2col planes + the split-precision GEMM: the layers the 3x3 stride-1 kernel cannot take --------
def conv_gemm_supported(conv, x):
    """Stride-1 / stride-2 square kernels (1x1, 3x3), any channel counts, fp32 device tensors: the UNet's and the VAE
    encoder's down-samplers, conv_in / conv_out (3, 4, 8, 9 channels), quant_conv."""
    if not (isinstance(conv, torch.nn.Conv2d) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if torch.is_grad_enabled() and (conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad)):
        return False                                  # frozen networks only: no parameter gradients here
    kh, kw = conv.kernel_size
    return (kh == kw and kh in (1, 3) and conv.stride[0] == conv.stride[1] and conv.stride[0] in (1, 2)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.weight.dtype == torch.float32
            and isinstance(conv.padding, tuple) and conv.padding_mode == 'zeros')


def _up(v, m):
    return (v + m - 1) // m * m


def _conv_gemm_packed(conv):
    """(A forward [MP x KP], A transposed [KP x MP], bias padded to MP): the weight as [Cout][Cin*KH*KW], zero padded
    to the GEMM's multiples of 32, packed once per (frozen) layer."""
    cache = conv.__dict__.setdefault('_mvip_packed_gemm', {})
    key = (conv.weight.data_ptr(), conv.weight._version)
    if cache.get('key') != key:
        cache.clear()
        cache['key'] = key
        Cout, K = conv.out_channels, conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
        MP, KP = _up(Cout, 32), _up(K, 32)
        w = torch.zeros((MP, KP), device=conv.weight.device, dtype=torch.float32)
        w[:Cout, :K] = conv.weight.detach().reshape(Cout, K)
        cache['fwd'] = gemm_pack_a(w, MP, KP, KP, 1, weights=True)
        cache['bwd'] = gemm_pack_a(w, KP, MP, 1, KP, weights=True)
        b = torch.zeros(MP, device=w.device, dtype=torch.float32)
        if conv.bias is not None:
            b[:Cout] = conv.bias.detach()
        cache['bias'] = b
    return cache['fwd'], cache['bwd'], cache['bias']


class _ConvGemm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, conv, pads):
        ctx.prec = _prec()
        if conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad):
            raise NotImplementedError('conv_gemm: parameter gradients are not implemented (frozen networks only)')
        xc = _f32c(x)
        N, Cin, H, W = xc.shape
        k, st = conv.kernel_size[0], conv.stride[0]
        pt, pl, pb, pr = pads
        OH, OW = (H + pt + pb - k) // st + 1, (W + pl + pr - k) // st + 1
        Cout, K = conv.out_channels, Cin * k * k
        MP, KP, P, PP = _up(Cout, 32), _up(K, 32), OH * OW, _up(OH * OW, 256)
        a_fwd, _, bias = _conv_gemm_packed(conv)
        s2 = unit_scale(xc.device) if forward_unit_scale() else absmax_scale(xc)
        xs = _split_buffer(N, KP, PP, xc.device)
        call('mvip_im2col_split_planes', ptr(xc), N, Cin, H, W, k, k, st, pt, pl, OH, OW, KP, PP, ptr(s2),
             ptr(xs, torch.float16), _prec(), stream())
        y = gemm_f16x3(xs, a_fwd, N, KP, MP, PP, bias=bias, x_scale2=s2)
        del xs
        ctx.conv, ctx.geom = conv, (N, Cin, H, W, k, st, pt, pl, OH, OW, Cout, MP, KP, P, PP)
        if MP != Cout or PP != P:
            y = y[:, :Cout, :P]
        return y.reshape(N, Cout, OH, OW)

    @staticmethod
    @_with_saved_prec
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        N, Cin, H, W, k, st, pt, pl, OH, OW, Cout, MP, KP, P, PP = ctx.geom
        d = _f32c(dy).reshape(N, Cout, P)
        if MP != Cout or PP != P:
            dp = torch.zeros((N, MP, PP), device=d.device, dtype=torch.float32)
            dp[:, :Cout, :P] = d
            d = dp
        _, a_bwd, _ = _conv_gemm_packed(ctx.conv)
        ds, s2 = _scaled_planes(d, N, MP, PP, MP * PP, PP, 1)
        col = gemm_f16x3(ds, a_bwd, N, MP, KP, PP, x_scale2=s2)                 # [N, KP, PP]
        del ds
        dx = torch.empty((N, Cin, H, W), device=d.device, dtype=torch.float32)
        call('mvip_col2im', ptr(col), N, Cin, H, W, k, k, st, pt, pl, OH, OW, KP, PP, ptr(dx), stream())
        return dx, None, None


def conv_gemm(x, conv, pads=None):
    """conv(x) + bias for the layers conv_gemm_supported accepts; `pads` = (top, left, bottom, right) overrides the
    module's symmetric padding (the VAE down-samplers pad bottom / right only).  Differentiable w.r.t. x."""
    if pads is None:
        pads = (conv.padding[0], conv.padding[1], conv.padding[0], conv.padding[1])
    return _ConvGemm.apply(x, conv, tuple(int(v) for v in pads))


def norm_conv1x1(x, norm, conv, ln_stats=False):
    """conv1x1(group_norm(x)) + bias, forward only (the UNet's transformer proj_in; runs under no_grad).
    ln_stats: as gemm_f16x3's (returns (y, stats))."""
    xc = x.detach().contiguous()
    N, C, H, W = xc.shape
    L, G, dev = H * W, norm.num_groups, xc.device
    ws = _gn_workspace(N, C, L, dev)
    xs = _split_buffer(N, C, L, dev)
    gw, gb = norm.weight.detach().contiguous(), norm.bias.detach().contiguous()
    if C // G < 4:
        mean, rstd = _gn_stats(xc, N, C, H, W, G, norm.eps, ws)
        call('mvip_groupnorm_split_planes', ptr(xc), ptr(gw), ptr(gb), ptr(mean), ptr(rstd), N, C, L, G, 0,
             ptr(xs, torch.float16), _prec(), stream())
    else:           # forward only: the plane writer reduces the moment partials itself
        rm = _row_moments_of(xc)
        if rm is None:
            call('mvip_groupnorm_stats', ptr(xc), N, C, L, G, float(norm.eps), 0, None, None, ptr(ws, torch.float64), stream())
            rm = ws
        call('mvip_groupnorm_split_planes_moments', ptr(xc), ptr(gw), ptr(gb), ptr(rm, torch.float64), float(norm.eps),
             N, C, L, G, 0, ptr(xs, torch.float16), _prec(), stream())
    bias = None if conv.bias is None else conv.bias.detach().contiguous()
    return gemm_f16x3(xs, _conv1x1_packed(conv, False), N, C, conv.out_channels, L, bias=bias, ln_stats=ln_stats)     # [N, Cout, L]


def tokens_conv1x1(h, conv, residual):
    """conv1x1 of token-major activations h [N, L, Cin] back to channel-first, + bias + residual [N, Cout, H, W];
    forward only (the UNet's transformer proj_out).  The token -> channel-first permute is folded into the
    split-plane writer's strides."""
    hc = h.detach().contiguous()
    N, L, C = hc.shape
    xs, s2 = _scaled_planes(hc, N, C, L, L * C, 1, C)
    bias = None if conv.bias is None else conv.bias.detach().contiguous()
    rs = residual.detach().contiguous()
    return gemm_f16x3(xs, _conv1x1_packed(conv, False), N, C, conv.out_channels, L, bias=bias, residual=rs,
                      x_scale2=s2).reshape(rs.shape)


# Transformer blocks of the SDS UNet: attention and token-side kernels (csrc/attention.hip, csrc/transformer.hip) -----

_ZERO_WORDS = {}
ZERO_SCOPE = None      # set by a hipGraph capture (guidance/sd_utils._GraphedStep) to a token of its own: every capture runs on
                       # torch's ONE shared capture stream, so without it all captured steps would bake in the SAME scratch words
                       # -- harmless while graphs replay one after the other, a race once two of them replay on different streams


def _zero_words(device):
    """64 scratch words per (device, stream[, capturing graph]) that are zero between kernel launches: the absmax collectors
    use them with atomics and the kernel that reads the maximum re-zeroes them (saves a zeroing launch per use)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, ZERO_SCOPE)
    if key not in _ZERO_WORDS:
        _ZERO_WORDS[key] = torch.zeros(64, device=device, dtype=torch.int32)
    return _ZERO_WORDS[key]


def absmax_scale_sections(x, outer, sections, length):
    """x viewed as [outer][sections][length] -> flat [sections * 4] device floats: {2^k, 2^-k, -, -} per section."""
    sc = torch.empty(sections * 4, device=x.device, dtype=_F32)
    call('mvip_absmax_scale_sections', ptr(x), int(outer), int(sections), int(length), ptr(sc),
         ptr(_zero_words(x.device), torch.int32), stream())
    return sc


def layernorm_split(x, weight, bias, eps, N, C, L, LP, out_scale, stats=None):
    """LayerNorm over the channel axis of channel-major x [N, C, LP] (tokens < L), times the power of two
    `out_scale`, as fp16 hi/lo split planes (the B operand of gemm_f16x3 with P = LP).  stats: the (partial moments,
    segments) pair the GEMM that produced x left (gemm_f16x3(..., ln_stats=True)): the statistics launch is skipped."""
    xs = _split_buffer(N, C, LP, x.device)
    if stats is not None:
        part, S = stats
        call('mvip_layernorm_split_planes_stats', ptr(x), ptr(weight), ptr(bias), ptr(part, torch.float64), int(S), int(N), int(C),
             int(L), int(LP), float(eps), float(out_scale), ptr(xs, torch.float16), _prec(), stream())
        return xs
    ws = torch.empty(int(_lib.load().mvip_layernorm_workspace_bytes(N, C, LP)) // 8, device=x.device, dtype=torch.float64)
    call('mvip_layernorm_split_planes', ptr(x), ptr(weight), ptr(bias), int(N), int(C), int(L), int(LP), float(eps),
         float(out_scale), ptr(ws, torch.float64), ptr(xs, torch.float16), _prec(), stream())
    return xs


def attention_pack_v(v, N, heads, D, DP, Lk, LkP, sn, sr, sk, scale2):
    """v.flatten()[n*sn + (h*DP + d)*sr + key*sk] -> the attention kernel's V operand (A fragments, fp16 hi/lo)."""
    nbytes = int(_lib.load().mvip_attention_v_bytes(N, heads, D, LkP))
    vp = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    call('mvip_attention_pack_v', ptr(v), int(N), int(heads), int(D), int(DP), int(Lk), int(LkP), int(sn), int(sr),
         int(sk), ptr(scale2), ptr(vp, torch.uint8), _prec(), stream())
    return vp


ATTENTION_FLAGS = 0      # bit 0: 64-key LDS tiles for 40-channel heads (A/B timing switch)


def attention_f16x3(qs, ks, vp, q_scale2, k_scale2, v_scale2, N, heads, D, Lq, LqP, Lk, LkP, out=None):
    """softmax(q k^T / sqrt(D)) v per head on the split-precision flash kernel -> fp32 [N, heads*D, LqP]
    (columns < Lq written; allocate `out` zeroed when LqP > Lq)."""
    if out is None:
        mk = torch.empty if LqP == Lq else torch.zeros
        out = mk((N, heads * D, LqP), device=qs.device, dtype=_F32)
    call('mvip_attention_f16x3', ptr(qs, torch.float16), ptr(ks, torch.float16), ptr(vp, torch.uint8), ptr(q_scale2),
         ptr(k_scale2), ptr(v_scale2), int(N), int(heads), int(D), int(Lq), int(LqP), int(Lk), int(LkP),
         float(D) ** -0.5, int(ATTENTION_FLAGS), ptr(out), _prec(), stream())
    return out


def geglu(y, N, R, L, LP):
    """y [N, 2R, LP] -> (y[:, :R] * gelu(y[:, R:]) [N, R, LP] zero beyond L, its power-of-two scale2)."""
    out = torch.empty((N, R, LP), device=y.device, dtype=_F32)
    scale2 = torch.empty(4, device=y.device, dtype=_F32)
    call('mvip_geglu', ptr(y), int(N), int(R), int(L), int(LP), ptr(out), ptr(scale2),
         ptr(_zero_words(y.device), torch.int32), stream())
    return out, scale2


def geglu_interleave(weight, bias):
    """[2R, K] weight / [2R] bias of a GEGLU projection (value rows, then gate rows) -> the same rows interleaved in
    32-row tiles (value tile t, gate tile t), the order `gemm_geglu_f16x3` expects."""
    R = weight.shape[0] // 2
    w = torch.stack([weight[:R].reshape(R // 32, 32, -1), weight[R:].reshape(R // 32, 32, -1)], 1).reshape(2 * R, -1)
    b = torch.stack([bias[:R].reshape(R // 32, 32), bias[R:].reshape(R // 32, 32)], 1).reshape(2 * R)
    return w.contiguous(), b.contiguous()


def gemm_geglu_f16x3(xs, packed, bias, N, K, M2, P, L, x_scale2=None):
    """(value * gelu(gate)) of the interleaved projection `packed` applied to split planes xs -> ([N, M2/2, P] fp32,
    its power-of-two scale2); columns >= L are zero."""
    out = torch.empty((N, M2 // 2, P), device=xs.device, dtype=_F32)
    scale2 = torch.empty(4, device=xs.device, dtype=_F32)
    call('mvip_gemm_geglu_f16x3', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(x_scale2), int(N),
         int(K), int(M2), int(P), int(L), ptr(out), ptr(scale2), ptr(_zero_words(xs.device), torch.int32), _prec_w(packed), stream())
    return out, scale2


def linear_small(x, W, b, act_in=0):
    """act(x) @ W^T + b for x [NB <= 8, K] in exact fp32 (act_in: 0 identity, 1 SiLU)."""
    xc, Wc = _f32c(x), _f32c(W)
    NB, K = xc.shape
    M = Wc.shape[0]
    y = torch.empty((NB, M), device=xc.device, dtype=_F32)
    call('mvip_linear_small', ptr(xc), ptr(Wc), ptr(None if b is None else _f32c(b)), NB, M, K, int(act_in), ptr(y),
         stream())
    return y


# Contractions that hand each other operands (csrc/plane_sink.h): the producer's epilogue writes the consumer's operand
# format at a power-of-two scale fixed before the launch ------------------------------------------------------------------

def pow2_scale_for_bound(bound, top=32768.0):
    """Largest power of two s with bound * s <= top (fp16 overflows at 65504; the hi/lo pair keeps ~2^-25 of `top`
    absolutely, i.e. fp32-grade accuracy relative to the tensor's maximum while the bound is < ~2^15 too wide)."""
    import math
    if not (bound > 0.0) or not math.isfinite(bound):
        return 1.0
    k = int(math.floor(math.log2(top / bound)))
    return float(2.0 ** max(-60, min(60, k)))


def scale2_tensor(s, device):
    return torch.tensor([s, 1.0 / s, 0.0, 0.0], device=device, dtype=_F32)


def gemm_f16x3_sinks(xs, packed, N, K, P, sections, bias=None, x_scale2=None, v_dt=1):
    """(W X + bias) with the rows cut into `sections` = [(rows, kind, scale), ...]: kind 'planes' -> fp16 hi/lo split
    planes [N][rows/16][2][2][P][8], kind 'vfrag' (last section only) -> attention V fragments
    [N][rows/(32 v_dt)][v_dt][P/16][2][64][8]; returns the list of operand buffers (uint8 / fp16 storage)."""
    import ctypes
    n = len(sections)
    M = sum(r for r, _, _ in sections)
    rows = (ctypes.c_int64 * n)(*[int(r) for r, _, _ in sections])
    kinds = (ctypes.c_int * n)(*[1 if k == 'planes' else 2 for _, k, _ in sections])
    scales = (ctypes.c_float * n)(*[float(sc) for _, _, sc in sections])
    bufs = []
    for r, k, _ in sections:
        if k == 'planes':
            bufs.append(_split_buffer(N, r, P, xs.device))                          # 4 B per element: fp16 hi + lo
        else:
            bufs.append(torch.empty(N * r * P * 4, device=xs.device, dtype=torch.uint8))
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    call('mvip_gemm_f16x3_sinks', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(x_scale2), int(N), int(K),
         int(M), int(P), n, rows, kinds, ptrs, scales, int(v_dt), _prec_w(packed), stream())
    return bufs


def gemm_geglu_f16x3_sink(xs, packed, bias, N, K, M2, P, L, out_scale, x_scale2=None):
    """(value * gelu(gate)) * out_scale of the interleaved projection as the second projection's operand planes
    [N][(M2/2)/16][2][2][P][8]; columns >= L are zero."""
    out = _split_buffer(N, M2 // 2, P, xs.device)
    call('mvip_gemm_geglu_f16x3_sink', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(x_scale2), int(N),
         int(K), int(M2), int(P), int(L), ptr(out, torch.float16), float(out_scale), _prec_w(packed), stream())
    return out


def attention_f16x3_sink(qs, ks, vp, q_scale2, k_scale2, v_scale2, N, heads, D, Lq, LqP, Lk, LkP, q_stride, k_stride,
                         v_groups):
    """mvip_attention_f16x3 on operands written by GEMM epilogues; the result leaves as the output projection's operand
    planes [N][heads*D/16][2][2][LqP][8], scaled by V's scale (zero beyond Lq when LqP > Lq)."""
    mk = torch.empty if LqP == Lq else torch.zeros
    out = mk(N * heads * D * LqP * 2, device=qs.device, dtype=torch.float16)
    call('mvip_attention_f16x3_sink', ptr(qs, torch.float16), ptr(ks, torch.float16), ptr(vp, torch.uint8), ptr(q_scale2),
         ptr(k_scale2), ptr(v_scale2), int(N), int(heads), int(D), int(Lq), int(LqP), int(Lk), int(LkP), int(q_stride),
         int(k_stride), int(v_groups), float(D) ** -0.5, int(ATTENTION_FLAGS), ptr(out, torch.float16), _prec(), stream())
    return out


def gemm_f16x3_planes(xs, packed, N, K, M, P, out_scale, bias=None, residual=None, x_scale2=None):
    """(W X + bias + residual) * out_scale as split planes [N][M/16][2][2][P][8] (the next GEMM's operand); split-K as
    gemm_f16x3 for the small grids."""
    out = _split_buffer(N, M, P, xs.device)
    nbytes = int(_lib.load().mvip_gemm_workspace_bytes(N, K, M, P))
    ws = torch.empty(nbytes // 4, device=xs.device, dtype=torch.float32) if nbytes else None
    call('mvip_gemm_f16x3_planes_ws', ptr(xs, torch.float16), ptr(packed, torch.uint8), ptr(bias), ptr(residual), ptr(x_scale2),
         int(N), int(K), int(M), int(P), ptr(out, torch.float16), float(out_scale), ptr(ws), _prec_w(packed), stream())
    return out


def linear_small_grouped(x, Wcat, bcat, offsets_dev, sizes, act_in=0):
    """act(x) @ W_l^T + b_l for several layers sharing x [NB <= 8, K] in ONE launch; returns one contiguous [NB, C_l]
    tensor per layer (views of one buffer).  Wcat [sum C_l, K], offsets_dev int32 [L + 1] on the device."""
    xc = _f32c(x)
    NB, K = xc.shape
    M = Wcat.shape[0]
    y = torch.empty(NB * M, device=xc.device, dtype=_F32)
    call('mvip_linear_small_grouped', ptr(xc), ptr(Wcat), ptr(bcat), NB, M, K, int(act_in), ptr(offsets_dev, torch.int32),
         len(sizes), ptr(y), stream())
    out, o = [], 0
    for c in sizes:
        out.append(y[o * NB:(o + c) * NB].view(NB, c))
        o += c
    return out


# render_rays in two launches (csrc/mlp_fwd16.hip, FUSE = 1 / 2): no-grad renders of the native networks ----------------

def render_coarse_fused(packed16, rows, lindisp, t_rand, noise, u, white_bkgd, need_alpha=False):
    """Coarse pass of render_rays (64 samples) behind ONE launch: stratified depths -> network -> raw2outputs -> inverse-CDF
    resampling (u: [B, Nf] or a shared row [Nf], Nf <= 64) -> merged depths.  Returns (rgb0, disp0, acc0, alpha0 | None,
    z_merged [B, 64 + Nf], z_std), bit-identical to stratified_z -> mlp_rays -> composite -> sample_pdf_merge."""
    rows = _f32c(rows)
    B, dev = rows.shape[0], rows.device
    u = _f32c(u)
    Nf = u.shape[-1]
    rgb = torch.empty((B, 3), device=dev, dtype=_F32)
    disp = torch.empty((B,), device=dev, dtype=_F32)
    acc = torch.empty((B,), device=dev, dtype=_F32)
    alpha = torch.empty((B, 64), device=dev, dtype=_F32) if need_alpha else None
    zm = torch.empty((B, 64 + Nf), device=dev, dtype=_F32)
    zstd = torch.empty((B,), device=dev, dtype=_F32)
    tr = None if t_rand is None else _f32c(t_rand)
    nz = None if noise is None else _f32c(noise)
    call('mvip_render_coarse_fused' + _fold16(packed16), ptr(packed16), ptr(rows), B, ptr(_t_vals(64, dev)), int(bool(lindisp)), ptr(tr), ptr(nz),
         ptr(u), int(u.dim() == 1), int(Nf), COMP_WHITE if white_bkgd else 0, ptr(rgb), ptr(disp), ptr(acc), ptr(None),
         ptr(None), ptr(alpha), ptr(zm), ptr(zstd), stream())
    return rgb, disp, acc, alpha, zm, zstd


def render_fine_fused(packed16, rows, z, noise, white_bkgd, need_alpha=False, want_raw=False):
    """Fine pass of render_rays (128 samples at depths z) behind ONE launch: network -> raw2outputs.  Returns (rgb, disp,
    acc, weights, depth, alpha | None, raw | None), bit-identical to mlp_rays -> composite."""
    rows, z = _f32c(rows), _f32c(z)
    B, dev = rows.shape[0], rows.device
    rgb = torch.empty((B, 3), device=dev, dtype=_F32)
    disp = torch.empty((B,), device=dev, dtype=_F32)
    acc = torch.empty((B,), device=dev, dtype=_F32)
    depth = torch.empty((B,), device=dev, dtype=_F32)
    weights = torch.empty((B, 128), device=dev, dtype=_F32)
    alpha = torch.empty((B, 128), device=dev, dtype=_F32) if need_alpha else None
    raw = torch.empty((B, 128, 4), device=dev, dtype=_F32) if want_raw else None
    nz = None if noise is None else _f32c(noise)
    call('mvip_render_fine_fused' + _fold16(packed16), ptr(packed16), ptr(rows), ptr(z), B, ptr(nz), COMP_WHITE if white_bkgd else 0, ptr(raw),
         ptr(rgb), ptr(disp), ptr(acc), ptr(depth), ptr(weights), ptr(alpha), stream())
    return rgb, disp, acc, weights, depth, alpha, raw


def softmax_rows(S, scale):
    """softmax(scale * S, -1) of a 2-D fp32 matrix on the HIP row kernel (the VAE mid-block attention's scores)."""
    Sc = _f32c(S)
    P = torch.empty_like(Sc)
    call('mvip_softmax_rows', ptr(Sc), Sc.shape[0], Sc.shape[1], float(scale), ptr(P), stream())
    return P


def softmax_rows_backward(P, dP, scale):
    """scale * P * (dP - rowsum(dP * P)): the adjoint of softmax_rows."""
    Pc, dc = _f32c(P), _f32c(dP)
    dS = torch.empty_like(Pc)
    call('mvip_softmax_rows_backward', ptr(Pc), ptr(dc), Pc.shape[0], Pc.shape[1], float(scale), ptr(dS), stream())
    return dS


# The 2D inpainting sampler (guidance/sd_utils.StableDiffusion.decode_latents / produce_latents / inpaint) ------------------

def vae_decoder_head(x, norm, conv, uint8=False):
    """clamp(conv(silu(norm(x))) / 2 + 0.5, 0, 1) for the VAE decoder's conv_norm_out / conv_out (3 output channels) and
    decode_latents' post-processing: GroupNorm statistics by one pass over x, then ONE launch (csrc/sd_sample.hip) that reads
    x once more -- no im2col planes.  Returns (img [N, 3, H, W] fp32, img_u8 [N, H, W, 3] = rint(255 img) or None).
    Forward only; `prec` is the current precision() (1 = the --fp16 mode's fp16 products)."""
    xc = _f32c(x.detach())
    N, C, H, W = xc.shape
    G, dev = norm.num_groups, xc.device
    if conv.out_channels != 3 or conv.in_channels != C or conv.kernel_size != (3, 3) or conv.padding != (1, 1):
        raise _lib.MvipError('vae_decoder_head: expects a 3x3 / padding 1 convolution to 3 channels')
    mean, rstd = _gn_stats(xc, N, C, H, W, G, norm.eps, _gn_workspace(N, C, H * W, dev))
    img = torch.empty((N, 3, H, W), device=dev, dtype=_F32)
    u8 = torch.empty((N, H, W, 3), device=dev, dtype=torch.uint8) if uint8 else None
    call('mvip_vae_decoder_head', ptr(xc), ptr(mean), ptr(rstd), ptr(_f32c(norm.weight.detach())), ptr(_f32c(norm.bias.detach())),
         ptr(_f32c(conv.weight.detach())), ptr(_f32c(conv.bias.detach())), N, C, H, W, G, 0, ptr(img),
         ptr(u8, torch.uint8), _prec(), stream())
    return img, u8


def ddim_cfg_step(eps, x, scal, unet_in=None, t_out=None):
    """One DDIM update (eta = 0) with classifier-free guidance in place on x [1, 4, h, w]: eps [2, 4, h, w] (uncond, cond) or
    [1, 4, h, w]; scal (device, 6 floats) = {g, sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev), t_next}.
    Also writes the new latents into channels 0..3 of the UNet input unet_in [1 + cfg, C_in, h, w] and t_next into t_out."""
    if not (x.is_contiguous() and x.dtype == _F32 and x.dim() == 4 and x.shape[:2] == (1, 4)):
        raise _lib.MvipError('ddim_cfg_step: x must be a dense fp32 [1, 4, h, w] tensor (updated in place)')
    e = _f32c(eps)
    hw = x.shape[2] * x.shape[3]
    cfg = e.shape[0] == 2
    if tuple(e.shape[1:]) != tuple(x.shape[1:]) or e.shape[0] not in (1, 2):
        raise _lib.MvipError(f'ddim_cfg_step: eps {tuple(e.shape)} does not match x {tuple(x.shape)}')
    if unet_in is not None and (unet_in.shape[0] != e.shape[0] or tuple(unet_in.shape[2:]) != tuple(x.shape[2:])):
        raise _lib.MvipError(f'ddim_cfg_step: UNet input {tuple(unet_in.shape)} does not match eps {tuple(e.shape)}')
    call('mvip_ddim_cfg_step', ptr(e), int(cfg), ptr(scal), ptr(x), hw, ptr(unet_in),
         0 if unet_in is None else unet_in.shape[1], ptr(t_out), stream())
    return x


# marching cubes (beyond the reference: mesh export, mvip_nerf_amd/mesh.py) -----------------------------

def marching_cubes(grid, iso, bound_min, bound_max, tri_table, valid=None):
    """grid [nx, ny, nz] fp32 on the device -> (verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32), csrc/mcubes.hip.
    tri_table: the 256 x 16 int8 device table of mesh.py.  Reads back the two totals and the non-finite flag once (the
    only synchronisation); raises ValueError for a non-finite grid, MvipError for more than 2^31 - 1 triangles.
    valid (None: every point): [nx, ny, nz] bool or uint8 on the grid's device, non-zero = observed; only cells whose eight
    corners are valid give triangles, only the edges around them vertices, and a point that is not valid may hold anything
    (mvip_mcubes_count_valid)."""
    g = _f32c(grid)
    nx, ny, nz = (int(s) for s in g.shape)
    dev = g.device
    if valid is not None:
        if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != tuple(g.shape):
            got = f'{tuple(valid.shape)} {valid.dtype}' if torch.is_tensor(valid) else type(valid).__name__
            raise ValueError(f'marching_cubes: valid must be a bool or uint8 tensor {tuple(g.shape)}, got {got}')
        if valid.device != dev:
            raise ValueError(f'marching_cubes: valid on {valid.device}, the grid on {dev}')
        valid = valid.detach().contiguous()
    G = _lib.load().mvip_mcubes_groups(nx, ny, nz)
    if G < 0:
        raise _lib.MvipError(f'marching_cubes: grid {tuple(g.shape)} outside 2..768 points per axis')
    flags = torch.empty(nx * ny * nz, device=dev, dtype=torch.int16)
    wg = torch.empty((G, 2), device=dev, dtype=torch.int64)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    if valid is None:
        call('mvip_mcubes_count', ptr(g), nx, ny, nz, float(iso), ptr(tri_table, torch.int8), ptr(flags, torch.int16),
             ptr(wg, torch.int64), ptr(totals, torch.int64), stream())
    else:
        call('mvip_mcubes_count_valid', ptr(g), ptr(valid, valid.dtype), nx, ny, nz, float(iso), ptr(tri_table, torch.int8),
             ptr(flags, torch.int16), ptr(wg, torch.int64), ptr(totals, torch.int64), stream())
    n_verts, n_tris, nonfinite = (int(x) for x in totals.cpu())
    if nonfinite:
        raise ValueError('marching_cubes: the grid holds a non-finite value' + (' at a valid point' if valid is not None else ''))
    if n_tris > 2 ** 31 - 1:
        raise _lib.MvipError(f'marching_cubes: {n_tris} triangles exceed int32 face indices')
    verts = torch.empty((n_verts, 3), device=dev, dtype=_F32)
    normals = torch.empty((n_verts, 3), device=dev, dtype=_F32)
    faces = torch.empty((n_tris, 3), device=dev, dtype=torch.int32)
    if n_verts or n_tris:
        vid = torch.empty(nx * ny * nz, device=dev, dtype=torch.int32)
        (x0, y0, z0), (x1, y1, z1) = ([float(v) for v in b] for b in (bound_min, bound_max))
        call('mvip_mcubes_emit', ptr(g), nx, ny, nz, float(iso), x0, y0, z0, x1, y1, z1, ptr(tri_table, torch.int8),
             ptr(flags, torch.int16), ptr(wg, torch.int64), n_verts, n_tris, ptr(vid, torch.int32), ptr(verts),
             ptr(normals), ptr(faces, torch.int32), stream())
    return verts, faces, normals


# occupancy-grid empty-space skipping (beyond the reference, mvip_nerf_amd/occupancy.py, csrc/occupancy.hip) -------------

_I32 = torch.int32


def occupancy_words(cells):
    """Number of int32 words of a grid of `cells` = (cx, cy, cz): one bit per cell, z fastest."""
    cx, cy, cz = (int(c) for c in cells)
    return (cx * cy * cz + 31) // 32


def _grid_args(who, box, cells, words, ok=True, shapes=''):
    """The grid's host-side arguments, after the check that `words` fits `cells`: box = (bmin[3], inv[3]) as six C floats,
    cells as three C ints.  ok / shapes: the caller's own shape check and its shapes, for the one message."""
    import ctypes
    if not ok or tuple(words.shape) != (occupancy_words(cells),):
        raise _lib.MvipError(f'{who}: {shapes}{tuple(words.shape)} words for cells {tuple(cells)}')
    return (ctypes.c_float * 6)(*[float(v) for v in box]), (ctypes.c_int * 3)(*[int(c) for c in cells])


def _grid_lookup(who, pts, box, cells, words):
    p = _f32c(pts.reshape(-1, 3))
    cbox, ccells = _grid_args(who, box, cells, words)
    out = torch.empty(p.shape[0], device=p.device, dtype=torch.uint8)
    call('mvip_' + who, ptr(p), p.shape[0], cbox, ccells, ptr(words, _I32), ptr(out, torch.uint8), stream())
    return out


def occupancy_build(sigma, cells, samples_per_cell, threshold):
    """sigma [cx k + 1, cy k + 1, cz k + 1] fp32 on the device -> int32 words: a cell is occupied iff any of the
    (k + 1)^3 points it owns has !(sigma <= threshold)."""
    s = _f32c(sigma)
    cx, cy, cz = (int(c) for c in cells)
    k = int(samples_per_cell)
    if tuple(s.shape) != (cx * k + 1, cy * k + 1, cz * k + 1):
        raise _lib.MvipError(f'occupancy_build: sigma {tuple(s.shape)} for cells {(cx, cy, cz)} x {k} samples per cell')
    words = torch.empty(occupancy_words(cells), device=s.device, dtype=_I32)
    call('mvip_occupancy_build', ptr(s), cx, cy, cz, int(samples_per_cell), float(threshold), ptr(words, _I32), stream())
    return words


def occupancy_dilate(words, cells):
    """One round of 27-neighbour dilation (clipped at the faces): a new word tensor."""
    cx, cy, cz = (int(c) for c in cells)
    if tuple(words.shape) != (occupancy_words(cells),):
        raise _lib.MvipError(f'occupancy_dilate: {tuple(words.shape)} words for cells {(cx, cy, cz)}')
    out = torch.empty_like(words)
    call('mvip_occupancy_dilate', ptr(words, _I32), cx, cy, cz, ptr(out, _I32), stream())
    return out


def occupancy_compact(rows, z, box, cells, words, want_mask=False, want_pts=False):
    """The kept samples of a ray chunk, in ascending flat order s = ray * S + j: (idx int32 [K], pts [K, 3], dirs [K, 3],
    K, mask uint8 [B, S] | None, pts_full [B, S, 3] | None).  rows [B, 11], z [B, S]; box = (bmin, inv) six floats, cells
    three ints (host), words on the rows' device.  Reads K back once (the only synchronisation)."""
    rows, z = _f32c(rows), _f32c(z)
    B, S = z.shape
    dev = z.device
    cbox, ccells = _grid_args('occupancy_compact', box, cells, words, tuple(rows.shape) == (B, 11),
                              f'rows {tuple(rows.shape)}, z {tuple(z.shape)}, ')
    G = _lib.load().mvip_occupancy_groups(B, S)
    if G < 0:
        raise _lib.MvipError(f'occupancy_compact: {B} x {S} samples exceed int32 sample indices')
    mask = torch.empty((B, S), device=dev, dtype=torch.uint8) if want_mask else None
    full = torch.empty((B, S, 3), device=dev, dtype=_F32) if want_pts else None
    K = 0
    if B > 0:
        wg = torch.empty(G, device=dev, dtype=_I32)
        total = torch.empty(1, device=dev, dtype=torch.int64)
        call('mvip_occupancy_count', ptr(rows), ptr(z), B, S, cbox, ccells, ptr(words, _I32), ptr(wg, _I32),
             ptr(total, torch.int64), ptr(mask, torch.uint8), ptr(full), stream())
        K = int(total.cpu())
    idx = torch.empty(K, device=dev, dtype=_I32)
    pts = torch.empty((K, 3), device=dev, dtype=_F32)
    dirs = torch.empty((K, 3), device=dev, dtype=_F32)
    if K > 0:
        call('mvip_occupancy_emit', ptr(rows), ptr(z), B, S, cbox, ccells, ptr(words, _I32), ptr(wg, _I32), K,
             ptr(idx, _I32), ptr(pts), ptr(dirs), stream())
    return idx, pts, dirs, K, mask, full


def scatter_raw(raw_k, idx, shape):
    """raw [*shape, 4] fp32: raw_k [K, 4] at the flat samples idx [K], zeros elsewhere (the zero fill is part of the op)."""
    n = _numel(shape)
    K = int(idx.shape[0])
    raw_k = _f32c(raw_k)
    if tuple(raw_k.shape) != (K, 4):
        raise _lib.MvipError(f'scatter_raw: raw_k {tuple(raw_k.shape)} for {K} indices (4 channels expected)')
    raw = torch.empty(tuple(shape) + (4,), device=idx.device, dtype=_F32)
    call('mvip_scatter_raw', ptr(raw_k) if K else ptr(None), ptr(idx, _I32) if K else ptr(None), K, n, ptr(raw), stream())
    return raw


def occupancy_lookup(pts, box, cells, words):
    """keep(p) of pts [P, 3]: uint8 [P], 1 = outside the box or in an occupied cell."""
    return _grid_lookup('occupancy_lookup', pts, box, cells, words)


# regions: 3D-consistent inpainting masks (beyond the reference, mvip_nerf_amd/region.py, csrc/region.hip) -----------------
# The grid arguments are occupancy's; inside(p) = in the box AND bit set.

def region_mark(pts, box, cells, words):
    """OR the bit of every point of pts [P, 3] that lies in the box into `words` (in place; returns words)."""
    p = _f32c(pts.reshape(-1, 3))
    cbox, ccells = _grid_args('region_mark', box, cells, words)
    call('mvip_region_mark', ptr(p), p.shape[0], cbox, ccells, ptr(words, _I32), stream())
    return words


def region_accumulate(rows, z, weights, box, cells, words):
    """out [B] = sum over j of (inside(rows[:, 0:3] + rows[:, 3:6] * z[:, j]) ? weights[:, j] : 0); rows [B, 11], z and
    weights [B, S].  No autograd: the inputs are read as they are."""
    rows, z, weights = _f32c(rows.detach()), _f32c(z.detach()), _f32c(weights.detach())
    B, S = z.shape
    cbox, ccells = _grid_args('region_accumulate', box, cells, words, tuple(rows.shape) == (B, 11) and tuple(weights.shape) == (B, S),
                              f'rows {tuple(rows.shape)}, z {tuple(z.shape)}, weights {tuple(weights.shape)}, ')
    out = torch.empty(B, device=z.device, dtype=_F32)
    call('mvip_region_accumulate', ptr(rows), ptr(z), ptr(weights), B, S, cbox, ccells, ptr(words, _I32), ptr(out), stream())
    return out


def region_lookup(pts, box, cells, words):
    """inside(p) of pts [P, 3]: uint8 [P], 1 = in the box and in a cell of the region."""
    return _grid_lookup('region_lookup', pts, box, cells, words)


# connected components of a bit array (beyond the reference, csrc/components.hip; bitgrid.py and mesh.py use them) --------
# The array is [nx, ny, nz], z fastest, 1..768 per axis, in the bit layout of the grids above.

CONNECTIVITIES = (6, 26)
MAX_COMPONENT_AXIS = 768


def _component_shape(who, shape, connectivity=6):
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f'{who}: connectivity must be 6 or 26, got {connectivity!r}')
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or not all(1 <= s <= MAX_COMPONENT_AXIS for s in shape):
        raise _lib.MvipError(f'{who}: shape {shape} outside three axes of 1..{MAX_COMPONENT_AXIS}')
    return shape


def grid_pack(values, threshold):
    """fp32 values (any shape, at most 768^3 elements) on the device -> int32 words [(n + 31) // 32]: bit l of the
    flattened array = values[l] >= threshold (NaN: clear), tail bits zero."""
    v = _f32c(values).reshape(-1)
    n = v.shape[0]
    threshold = float(threshold)
    if threshold != threshold or n > MAX_COMPONENT_AXIS ** 3:
        raise _lib.MvipError(f'grid_pack: {n} values, threshold {threshold} (at most 768^3 values, threshold not NaN)')
    words = torch.empty((n + 31) // 32, device=v.device, dtype=_I32)
    call('mvip_components_pack', ptr(v), n, threshold, ptr(words, _I32), stream())
    return words


def grid_components(words, shape, connectivity=6):
    """Connected components of the set bits of `words` read as an array of `shape` = (nx, ny, nz): (labels [nx, ny, nz]
    int32, sizes [n] int32, first [n] int32).  labels is 0 where the bit is clear and else the 1-based number of the
    element's component; components are numbered by ascending lowest linear index (`first`), the order of
    scipy.ndimage.label.  connectivity 6 (faces) or 26 (the 3 x 3 x 3 neighbourhood).  With no set bit labels is all zeros
    and sizes / first are empty.  Reads the number of components back once (the only synchronisation)."""
    nx, ny, nz = _component_shape('grid_components', shape, connectivity)
    n = nx * ny * nz
    if tuple(words.shape) != ((n + 31) // 32,):
        raise _lib.MvipError(f'grid_components: {tuple(words.shape)} words for shape {(nx, ny, nz)}')
    dev = words.device
    G = _lib.load().mvip_components_groups(nx, ny, nz)
    parent = torch.empty(n, device=dev, dtype=_I32)
    wg = torch.empty(G, device=dev, dtype=_I32)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    call('mvip_components_label', ptr(words, _I32), nx, ny, nz, int(connectivity), ptr(parent, _I32), ptr(wg, _I32),
         ptr(total, torch.int64), stream())
    nc = int(total.cpu())
    sizes = torch.empty(nc, device=dev, dtype=_I32)
    first = torch.empty(nc, device=dev, dtype=_I32)
    if nc == 0:
        return torch.zeros((nx, ny, nz), device=dev, dtype=_I32), sizes, first
    labels = torch.empty((nx, ny, nz), device=dev, dtype=_I32)
    call('mvip_components_rank', ptr(parent, _I32), nx, ny, nz, ptr(wg, _I32), nc, ptr(labels, _I32), ptr(sizes, _I32),
         ptr(first, _I32), stream())
    return labels, sizes, first


def grid_select(labels, keep):
    """labels (int32, any shape) and keep uint8 [n_components + 1] (keep[0] = 0) -> int32 words of exactly the elements
    whose component is kept, tail bits zero."""
    lab = labels.contiguous().reshape(-1)
    n = lab.shape[0]
    if keep.dim() != 1 or keep.shape[0] < 1 or keep.shape[0] - 1 > n or n > MAX_COMPONENT_AXIS ** 3:
        raise _lib.MvipError(f'grid_select: keep {tuple(keep.shape)} for {n} labels')
    if keep.shape[0] == 1 or n == 0:
        return torch.zeros((n + 31) // 32, device=lab.device, dtype=_I32)
    words = torch.empty((n + 31) // 32, device=lab.device, dtype=_I32)
    call('mvip_components_select', ptr(lab, _I32), n, ptr(keep.contiguous(), torch.uint8), keep.shape[0] - 1, ptr(words, _I32),
         stream())
    return words


def component_criteria(who, largest, min_size, other=False, size_name='min_cells'):
    """The checked (largest, min_size) of a keep-components call: each None or an integer >= 1, and at least one criterion
    given (`other`: the caller has one of its own).  ValueError otherwise; nothing is launched."""
    for name, v in (('largest', largest), (size_name, min_size)):
        if v is not None and (int(v) != v or int(v) < 1):
            raise ValueError(f'{who}: {name} must be an integer >= 1, got {v!r}')
    if largest is None and min_size is None and not other:
        raise ValueError(f'{who}: no criterion given: name the components to keep (largest, {size_name}, ...)')
    return (None if largest is None else int(largest)), (None if min_size is None else int(min_size))


def component_keep_table(sizes, largest=None, min_size=None, also=None):
    """keep uint8 [n + 1] (host numpy; keep[0] = 0) over components 1..n of sizes [n] (host, in label order, i.e. by
    ascending lowest index).  largest = k: the k components with the most elements, ties to the lower label (= the lower
    `first`); min_size = m: components of at least m elements; a component must meet every criterion given.  also: labels
    kept in any case (OR-ed in; 0 and out-of-range entries ignored).  With neither criterion only `also` is kept."""
    import numpy as np
    sizes = np.asarray(sizes, np.int64)
    n = sizes.shape[0]
    kept = np.zeros(n, bool)
    if largest is not None or min_size is not None:
        kept[:] = True
        if min_size is not None:
            kept &= sizes >= min_size
        if largest is not None:
            top = np.zeros(n, bool)
            top[np.argsort(-sizes, kind='stable')[:largest]] = True
            kept &= top
    if also is not None:
        a = np.asarray(also, np.int64).reshape(-1)
        kept[a[(a >= 1) & (a <= n)] - 1] = True
    table = np.zeros(n + 1, np.uint8)
    table[1:] = kept
    return table


# ray distortion loss (mip-NeRF 360 eq. 15; beyond the reference, csrc/distortion.hip) ------------------------------------------

class _DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, z, rows, lindisp):
        B, S = z.shape
        loss = torch.empty((B,), device=z.device, dtype=_F32)
        grad = torch.empty((B, S), device=z.device, dtype=_F32) if ctx.needs_input_grad[0] else None
        call('mvip_distortion_loss', ptr(rows), rows.shape[1], ptr(z), ptr(weights), B, S, int(bool(lindisp)), ptr(loss),
             ptr(grad), stream())
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        grad, = ctx.saved_tensors
        return g_loss[:, None] * grad, None, None, None


def distortion_loss(weights, z, rows, lindisp=False):
    """loss [B] = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_j w_j^2 d_j over the normalised intervals of z [B, S] (ascending
    along the ray; near / far from rows[:, 6:8], rows [B, 8] or [B, 11]; the conventions are csrc/distortion.hip's).  One
    launch; when `weights` requires grad the same launch writes d loss / d weights, and the backward is one elementwise
    product.  Gradient goes to `weights` only (the fine depths are detached resamples)."""
    if not (torch.is_tensor(weights) and torch.is_tensor(z) and torch.is_tensor(rows)) or z.dim() != 2 \
            or tuple(weights.shape) != tuple(z.shape) or rows.dim() != 2 or rows.shape[0] != z.shape[0] \
            or rows.shape[1] not in (8, 11) or z.shape[1] < 1:
        shape = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise _lib.MvipError(f'distortion_loss: weights {shape(weights)}, z {shape(z)}, rows {shape(rows)}')
    if not (weights.is_cuda and z.device == weights.device and rows.device == weights.device):
        raise _lib.MvipError(f'distortion_loss: weights on {weights.device}, z on {z.device}, rows on {rows.device}; the HIP '
                             'path has no CPU fallback')
    return _DistortionLoss.apply(_f32c(weights), _f32c(z.detach()), _f32c(rows.detach()), bool(lindisp))


# harmonic hole filling, its guided (Poisson) variant and 2D mask dilation (beyond the reference: stands in for --prepare + LaMa;
# csrc/harmonic.hip) ------------------------------------------------------------------------------------------------------------

def _image_batch(what, t, dtype, name):
    if not torch.is_tensor(t):
        raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
    if t.dtype != dtype:
        raise ValueError(f'{what}: {name} must be {dtype}, got {t.dtype}')
    if t.dim() != 3:
        raise ValueError(f'{what}: {name} must be [N, H, W], got {tuple(t.shape)}')
    if t.shape[0] > 0 and (t.shape[1] < 1 or t.shape[2] < 1):
        raise ValueError(f'{what}: empty images {tuple(t.shape)}')
    return t.detach()


def _on_gpu(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU fallback)')


def mask_dilate2d(masks, rounds):
    """masks [N, H, W] bool on the device -> bool: `rounds` rounds of "set iff any pixel at Chebyshev distance <= 1 is set",
    clipped at the border (the 2D twin of occupancy_dilate).  rounds = 0: a copy."""
    m = _image_batch('mask_dilate2d', masks, torch.bool, 'masks')
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError(f'mask_dilate2d: rounds must be >= 0, got {rounds}')
    _on_gpu('mask_dilate2d', m)
    m = m.contiguous()
    N, H, W = m.shape
    cur = m.clone()
    for _ in range(rounds if N else 0):
        nxt = torch.empty_like(cur)
        call('mvip_mask_dilate2d', ptr(cur, torch.bool), N, H, W, ptr(nxt, torch.bool), stream())
        cur = nxt
    return cur


HARMONIC_STATE_WORDS = 16


def harmonic_fill(values, masks, eps=1e-7, max_iters=None, check_every=32):
    """Fill the masked (and the non-finite) pixels of values [N, H, W] fp32 with the harmonic interpolant of the others: per
    image the discrete Laplace equation with a mirror boundary at the image border (the definition is csrc/harmonic.hip's
    and tests/harmonic_numpy.py's), by Jacobi-preconditioned conjugate gradients from zero until r.z <= eps^2 r0.z0.
    Returns (filled [N, H, W], info); info holds per image numpy arrays `unknowns`, `iterations`, `residual` (the true
    residual in the max norm, for the record: it stalls near 1e-6 in fp32 while the error still falls), `converged`,
    `singular` (every pixel unknown: returned unchanged).  Known finite pixels come back bit for bit.  max_iters=None means
    8 * max(H, W): a cap so that the call always ends (the counts measured are about 2.2 x the hole's diameter).  The flags
    are read back once every `check_every` iterations.  Detached: no autograd."""
    v, m = _fill_operands('harmonic_fill', values, masks)
    return _cg_fill('harmonic_fill', v, m, eps, max_iters, check_every,
                    lambda N, H, W, out, ws, state, max_act, st: call('mvip_harmonic_init', ptr(v), N, H, W, out, ws, state, max_act, st))


def poisson_fill(values, masks, guide, labels, eps=1e-7, max_iters=None, check_every=32):
    """harmonic_fill with a guidance field (gradient-domain / Poisson blending; the definition is csrc/harmonic.hip's and
    tests/poisson_numpy.py's): guide [N, H, W] fp32 and labels [N, H, W] int32 beside values and masks.  An edge between two
    4-neighbours is guided iff both carry the same label >= 0 and a finite guide; the unknowns then keep the guide's
    difference across every guided edge and the harmonic zero difference across every other one, with `values` on the known
    pixels as the boundary.  With no guided edge (labels -1, or a non-finite guide) the result is harmonic_fill's bit for
    bit.  Returns (filled, info) as harmonic_fill does; the same solver, the same caps, detached."""
    v, m = _fill_operands('poisson_fill', values, masks)
    g = _image_batch('poisson_fill', guide, _F32, 'guide')
    l = _image_batch('poisson_fill', labels, _I32, 'labels')
    if tuple(g.shape) != tuple(v.shape) or tuple(l.shape) != tuple(v.shape) or g.device != v.device or l.device != v.device:
        raise ValueError(f'poisson_fill: values {tuple(v.shape)} on {v.device}, guide {tuple(g.shape)} on {g.device}, labels '
                         f'{tuple(l.shape)} on {l.device}')
    if not g.is_contiguous():
        raise ValueError('poisson_fill: guide must be contiguous')
    l = l.contiguous()                                               # (on values' device, which the shared loop holds to a GPU)
    return _cg_fill('poisson_fill', v, m, eps, max_iters, check_every,
                    lambda N, H, W, out, ws, state, max_act, st: call('mvip_poisson_init', ptr(v), ptr(g), ptr(l, _I32), N, H, W, out, ws,
                                                                      state, max_act, st))


def _fill_operands(what, values, masks):
    v = _image_batch(what, values, _F32, 'values')
    m = _image_batch(what, masks, torch.bool, 'masks')
    if tuple(v.shape) != tuple(m.shape) or v.device != m.device:
        raise ValueError(f'{what}: values {tuple(v.shape)} on {v.device}, masks {tuple(m.shape)} on {m.device}')
    if not v.is_contiguous():
        raise ValueError(f'{what}: values must be contiguous')
    return v, m


def _cg_fill(what, v, m, eps, max_iters, check_every, init):
    """The driving loop of harmonic_fill and poisson_fill: set-up, `init` (the right-hand side: the one call in which the two
    differ; it gets N, H, W, the out / workspace / state pointers, max_act and the stream), iterations with a read-back every
    check_every, the verdict."""
    import numpy as np
    N, H, W = v.shape
    eps, check_every = float(eps), int(check_every)
    max_iters = 8 * max(H, W) if max_iters is None else int(max_iters)
    if not 0.0 <= eps < 1.0 or max_iters < 0 or check_every < 1:
        raise ValueError(f'{what}: eps {eps} (0 <= eps < 1), max_iters {max_iters} (>= 0), check_every {check_every} (>= 1)')
    _on_gpu(what, v, m)
    m = m.contiguous()
    out = torch.empty_like(v)
    if N == 0:
        e = np.zeros(0, np.int64)
        return out, {'unknowns': e, 'iterations': e.copy(), 'residual': np.zeros(0, np.float32),
                     'converged': np.zeros(0, bool), 'singular': np.zeros(0, bool)}
    nbytes = _lib.load().mvip_harmonic_workspace_bytes(N, H, W)
    if nbytes < 0:
        raise ValueError(f'{what}: {N} images of {H} x {W} are beyond the kernels\' index range')
    ws = torch.empty(nbytes, device=v.device, dtype=torch.uint8)
    state = torch.empty((N, HARMONIC_STATE_WORDS), device=v.device, dtype=_I32)
    st = stream()
    call('mvip_harmonic_setup', ptr(v), ptr(m, torch.bool), N, H, W, ptr(out), ptr(ws, torch.uint8), ptr(state, _I32), st)
    max_act = int(state[:, 0].max().cpu())                           # read-back: sizes the launches over the active tiles
    if max_act > 0:
        init(N, H, W, ptr(out), ptr(ws, torch.uint8), ptr(state, _I32), max_act, st)
        k = 0
        while k < max_iters:
            n = min(check_every, max_iters - k)
            call('mvip_harmonic_iterate', N, H, W, ptr(out), ptr(ws, torch.uint8), ptr(state, _I32), max_act, k, n, eps, st)
            k += n
            if bool(state[:, 3].all().cpu()):                        # read-back: every image is frozen
                break
    call('mvip_harmonic_finish', N, H, W, ptr(out), ptr(ws, torch.uint8), ptr(state, _I32), max_act, eps, st)
    s = state.cpu().numpy()
    info = {'unknowns': s[:, 1].astype(np.int64), 'iterations': s[:, 4].astype(np.int64),
            'residual': np.ascontiguousarray(s[:, 8]).view(np.float32).copy(), 'converged': s[:, 9] != 0, 'singular': s[:, 2] != 0}
    return out, info


# reference-view propagation: backward depth warping (beyond the reference, which has no counterpart; csrc/warp.hip) --------------

def _pose_batch(what, t, name):
    if not torch.is_tensor(t):
        raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
    if t.dtype != _F32:
        raise ValueError(f'{what}: {name} must be {_F32}, got {t.dtype}')
    if t.dim() != 3 or tuple(t.shape[1:]) != (3, 4):
        raise ValueError(f'{what}: {name} must be [N, 3, 4], got {tuple(t.shape)}')
    return t.detach()


def _view_batch(what, disp, poses, masks):
    """disp [V, H, W] fp32, poses [V, 3, 4] and the optional masks [V, H, W] bool of one V -> (d, p, m or None), detached."""
    d = _image_batch(what, disp, _F32, 'disp')
    p = _pose_batch(what, poses, 'poses')
    if p.shape[0] != d.shape[0]:
        raise ValueError(f'{what}: disp {tuple(d.shape)}, poses {tuple(p.shape)}: one V expected')
    m = None
    if masks is not None:
        m = _image_batch(what, masks, torch.bool, 'masks')
        if tuple(m.shape) != tuple(d.shape):
            raise ValueError(f'{what}: masks {tuple(m.shape)} for disp {tuple(d.shape)}')
    return d, p, m


def _views_ready(what, tensors, **scalars):
    """What every view operator checks last: the two scalars given by name (focal and the call's tolerance) finite and > 0,
    the operands on one GPU and contiguous.  Returns the scalars as floats."""
    (a, x), (b, y) = ((k, float(v)) for k, v in scalars.items())
    if not (0.0 < x < float('inf') and 0.0 < y < float('inf')):
        raise ValueError(f'{what}: {a} {x} and {b} {y} must be finite and > 0')
    _on_gpu(what, *tensors)
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(t.device) for t in tensors})}')
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: every operand must be contiguous')
    return x, y


def warp_views(tgt_disp, tgt_pose, tgt_mask, src_rgb, src_disp, src_pose, focal, order=None, tol=0.05):
    """Backward depth warp of S source views into N target views (the definition is csrc/warp.hip's and tests/warp_numpy.py's).
    tgt_disp [N, H, W] fp32, tgt_pose [N, 3, 4], tgt_mask [N, H, W] bool (the pixels to compute); src_rgb [S, H, W, 3],
    src_disp [S, H, W], src_pose [S, 3, 4]; order [N, S] int32: per target the sources in order of preference (None: ascending
    index), an entry outside [0, S) is skipped.  A masked pixel with a finite disparity > 0 takes the first source in which it
    projects inside the image, in front of the camera, and onto a surface at its own depth: |t_s d_s - 1| <= tol (0.05 sits above
    the step of 8-bit disparity rasters, 0.5 to 3 % of their value).  Returns (rgb [N, H, W, 3], index [N, H, W] int32: the
    source or -1, resid [N, H, W]); 0 / -1 / 0 where nothing is taken.  One launch.  Detached: no autograd."""
    what = 'warp_views'
    d = _image_batch(what, tgt_disp, _F32, 'tgt_disp')
    m = _image_batch(what, tgt_mask, torch.bool, 'tgt_mask')
    sd = _image_batch(what, src_disp, _F32, 'src_disp')
    tp, sp = _pose_batch(what, tgt_pose, 'tgt_pose'), _pose_batch(what, src_pose, 'src_pose')
    if not torch.is_tensor(src_rgb) or src_rgb.dtype != _F32 or src_rgb.dim() != 4 or src_rgb.shape[-1] != 3:
        got = f'{tuple(src_rgb.shape)} {src_rgb.dtype}' if torch.is_tensor(src_rgb) else type(src_rgb).__name__
        raise ValueError(f'{what}: src_rgb must be a {_F32} tensor [S, H, W, 3] on the GPU, got {got}')
    sc = src_rgb.detach()
    N, H, W = d.shape
    S = sd.shape[0]
    if tuple(m.shape) != (N, H, W) or tp.shape[0] != N:
        raise ValueError(f'{what}: tgt_disp {tuple(d.shape)}, tgt_mask {tuple(m.shape)}, tgt_pose {tuple(tp.shape)}: one N, H, W expected')
    if tuple(sd.shape[1:]) != (H, W) or tuple(sc.shape) != (S, H, W, 3) or sp.shape[0] != S:
        raise ValueError(f'{what}: src_disp {tuple(sd.shape)}, src_rgb {tuple(sc.shape)}, src_pose {tuple(sp.shape)} for targets of '
                         f'{H} x {W}: one S, and the targets\' H, W expected')
    if H < 2 or W < 2:
        raise ValueError(f'{what}: images of at least 2 x 2 expected, got {H} x {W}')
    tensors = [d, tp, m, sc, sd, sp]
    if order is not None:
        if not torch.is_tensor(order) or order.dtype != _I32 or tuple(order.shape) != (N, S):
            got = f'{tuple(order.shape)} {order.dtype}' if torch.is_tensor(order) else type(order).__name__
            raise ValueError(f'{what}: order must be an {_I32} tensor [{N}, {S}] on the GPU, got {got}')
        tensors.append(order.detach())
    focal, tol = _views_ready(what, tensors, focal=focal, tol=tol)
    if order is None:
        order = torch.arange(S, device=d.device, dtype=_I32).repeat(N, 1).reshape(N, S)
    rgb = torch.empty((N, H, W, 3), device=d.device, dtype=_F32)
    index = torch.empty((N, H, W), device=d.device, dtype=_I32)
    resid = torch.empty((N, H, W), device=d.device, dtype=_F32)
    call('mvip_warp_views', ptr(d), ptr(tp), ptr(m, torch.bool), N, H, W, ptr(sc), ptr(sd), ptr(sp), S, ptr(order.detach(), _I32),
         focal, tol, ptr(rgb), ptr(index, _I32), ptr(resid), stream())
    return rgb, index, resid


# TSDF fusion of depth maps (beyond the reference, which has no mesh export; csrc/tsdf.hip, mesh.fuse_depths) -----------------------

def tsdf_fuse(disp, poses, focal, bound_min, bound_max, resolution, trunc, masks=None):
    """Fuse V disparity maps into a truncated signed distance field on a lattice (the definition is csrc/tsdf.hip's and
    tests/tsdf_numpy.py's).  disp [V, H, W] fp32 (1 / planar depth, as prepare.render_disparities returns it), poses [V, 3, 4]
    camera-to-world, masks [V, H, W] bool (False: ignore the pixel) or None; bound_min / bound_max: three coordinates each;
    resolution: an int or three point counts (2..768 each); trunc: the truncation distance, finite and > 0.  Returns
    (tsdf [nx, ny, nz] fp32 in [-1, 1]: the mean over the views that see the point of min(1, (depth - z) / trunc), 1 where
    there is none; count [nx, ny, nz] int32: those views).  A view sees a point iff it projects onto a pixel (the nearest
    one) with a finite disparity > 0 and lies no more than trunc behind that pixel's surface.  One launch.  Detached."""
    import math
    import numpy as np
    what = 'tsdf_fuse'
    d, p, m = _view_batch(what, disp, poses, masks)
    V, H, W = d.shape
    if H < 1 or W < 1:
        raise ValueError(f'{what}: images of at least 1 x 1 expected, got {H} x {W}')
    focal, trunc = _views_ready(what, [d, p] if m is None else [d, p, m], focal=focal, trunc=trunc)
    lo = [float(np.float32(v)) for v in bound_min]
    hi = [float(np.float32(v)) for v in bound_max]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f'{what}: bound_min {lo} must be finite and below bound_max {hi} on every axis')
    res = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)
    if len(res) != 3 or not all(2 <= n <= MAX_COMPONENT_AXIS for n in res):
        raise ValueError(f'{what}: resolution {res}: three axes of 2..{MAX_COMPONENT_AXIS} points each')
    tsdf = torch.empty(res, device=d.device, dtype=_F32)
    count = torch.empty(res, device=d.device, dtype=_I32)
    call('mvip_tsdf_fuse', ptr(d), ptr(p), ptr(m, torch.bool), V, H, W, focal, res[0], res[1], res[2], lo[0], lo[1], lo[2],
         hi[0], hi[1], hi[2], trunc, ptr(tsdf), ptr(count, _I32), stream())
    return tsdf, count


# quantile ray depth and cross-view depth consistency (beyond the reference; csrc/ray_depth.hip, csrc/depth_consistency.hip) -------

RAY_DEPTH_MAX_SAMPLES = 4096
RAY_DEPTH_MAX_LEVELS = 8
RAY_DEPTH_FIX = 2.0 ** 40          # weights and levels are compared as integers in units of 2^-40


def _quantile_levels(what, levels):
    import ctypes
    import numpy as np
    try:
        lv = [float(np.float32(q)) for q in levels]
    except TypeError:
        raise ValueError(f'{what}: levels must be a sequence of numbers, got {type(levels).__name__}') from None
    if not 1 <= len(lv) <= RAY_DEPTH_MAX_LEVELS:
        raise ValueError(f'{what}: 1..{RAY_DEPTH_MAX_LEVELS} levels expected, got {len(lv)}')
    if not all(0.0 < q < 1.0 and int(np.floor(q * RAY_DEPTH_FIX)) >= 1 for q in lv):
        raise ValueError(f'{what}: every level must satisfy 0 < q < 1 (and q >= 2^-40), got {tuple(levels)}')
    return (ctypes.c_float * len(lv))(*lv)


def ray_quantile_depth(weights, z, levels=(0.5,)):
    """depth [B, Q] fp32: per ray and level q the depth at which the accumulated compositing weight reaches q (q = 0.5: the
    median termination depth), weights [B, S] and z [B, S] ascending along the ray, 1 <= S <= 4096, up to 8 levels (the
    definition, in integers and fp64, is csrc/ray_depth.hip's and tests/ray_depth_numpy.py's).  +inf where the ray's weights
    never sum to q; the last sample's own depth when it is the crossing one; NaN at every level of a ray with a non-finite
    weight.  One launch for all levels.  Detached: no autograd."""
    what = 'ray_quantile_depth'
    if not (torch.is_tensor(weights) and torch.is_tensor(z)) or z.dim() != 2 or tuple(weights.shape) != tuple(z.shape) \
            or not 1 <= z.shape[1] <= RAY_DEPTH_MAX_SAMPLES:
        shape = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise _lib.MvipError(f'{what}: weights {shape(weights)}, z {shape(z)}: two [B, S] tensors with 1 <= S <= '
                             f'{RAY_DEPTH_MAX_SAMPLES} expected')
    lv = _quantile_levels(what, levels)
    if not (weights.is_cuda and z.device == weights.device):
        raise _lib.MvipError(f'{what}: weights on {weights.device}, z on {z.device}; the HIP path has no CPU fallback')
    B, S = z.shape
    if B * S > 2 ** 31 - 1:
        raise _lib.MvipError(f'{what}: {B} x {S} samples are beyond the kernel\'s index range')
    w, zz = _f32c(weights.detach()), _f32c(z.detach())
    depth = torch.empty((B, len(lv)), device=z.device, dtype=_F32)
    call('mvip_ray_quantile_depth', ptr(zz), ptr(w), B, S, lv, len(lv), ptr(depth), stream())
    return depth


def depth_consistency(disp, poses, focal, masks=None, tol=0.05):
    """(agree, violated), int32 [V, H, W]: per pixel of every view the number of OTHER views that see a surface at the
    pixel's world point (|t_s d_s - 1| <= tol) and the number that see through it to a farther surface (t_s d_s - 1 < -tol: a
    free-space violation, what a floater earns); an occluded point (residual > tol), one outside the other image or one
    that lands on an invalid pixel counts as neither.  disp [V, H, W] fp32 (1 / planar depth), poses [V, 3, 4]
    camera-to-world, masks [V, H, W] bool or None: a False pixel is zeroed before the launch, so it is neither judged nor a
    witness.  The definition (fp64, the conventions and the default tol of warp_views) is csrc/depth_consistency.hip's and
    tests/depth_consistency_numpy.py's.  One launch.  Detached."""
    what = 'depth_consistency'
    d, p, m = _view_batch(what, disp, poses, masks)
    V, H, W = d.shape
    if H < 2 or W < 2 or H > RASTER_MAX_SIDE or W > RASTER_MAX_SIDE:
        raise ValueError(f'{what}: images of 2..{RASTER_MAX_SIDE} pixels a side expected, got {H} x {W}')
    focal, tol = _views_ready(what, [d, p] if m is None else [d, p, m], focal=focal, tol=tol)
    if m is not None:
        d = torch.where(m, d, torch.zeros((), device=d.device, dtype=_F32)).contiguous()
    agree = torch.empty((V, H, W), device=d.device, dtype=_I32)
    violated = torch.empty((V, H, W), device=d.device, dtype=_I32)
    call('mvip_depth_consistency', ptr(d), ptr(p), V, H, W, focal, tol, ptr(agree, _I32), ptr(violated, _I32), stream())
    return agree, violated


# structural similarity with its gradient (beyond the reference, whose evaluation.py takes its metrics from pyiqa; csrc/ssim.hip) --

SSIM_WINDOW = 11                 # taps; the map is [N, H - 10, W - 10, C]
SSIM_TILE = (16, 32)             # map rows x columns per workgroup (csrc/ssim.hip: TY, TX)


class _Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mask, want_map):
        N, H, W, C = x.shape
        MH, MW = H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1
        dev = x.device
        need = ctx.needs_input_grad[0]
        tiles = _lib.load().mvip_ssim_tiles(H, W)
        if tiles < 0:
            raise _lib.MvipError(f'ssim: images of {H} x {W} are beyond the kernels\' index range')
        ssim = torch.empty((N,), device=dev, dtype=_F32)
        count = torch.empty((N,), device=dev, dtype=_I32)
        part = torch.empty((N * tiles,), device=dev, dtype=torch.float64)
        pcnt = torch.empty((N * tiles,), device=dev, dtype=_I32)
        smap = torch.empty((N, MH, MW, C), device=dev, dtype=_F32) if want_map else None
        stash = torch.empty((3, N, MH, MW, C), device=dev, dtype=_F32) if need else None
        call('mvip_ssim_forward', ptr(x), ptr(y), ptr(mask, torch.bool), N, H, W, C, ptr(smap), ptr(stash),
             ptr(part, torch.float64), ptr(pcnt, _I32), ptr(ssim), ptr(count, _I32), stream())
        if need:
            ctx.save_for_backward(x, y, stash, count)
        if smap is None:
            ctx.mark_non_differentiable(count)
            return ssim, count
        ctx.mark_non_differentiable(count, smap)
        return ssim, count, smap

    @staticmethod
    def backward(ctx, g_ssim, *_):
        x, y, stash, count = ctx.saved_tensors
        N, H, W, C = x.shape
        gx = torch.empty_like(x)
        call('mvip_ssim_backward', ptr(x), ptr(y), ptr(stash), ptr(_f32c(g_ssim)), ptr(count, _I32), N, H, W, C, ptr(gx), stream())
        return gx, None, None, None


def ssim(x, y, mask=None, return_map=False, return_count=False):
    """Structural similarity of x against y, per image: ssim [N] fp32, or (ssim, map [N, H-10, W-10, C]) with return_map (and
    count [N] int32, the counted map pixels, last with return_count).  x, y [N, H, W, C] fp32 on the GPU, contiguous,
    channel-last (what run.render and the scene hold), C in 1..4, H, W >= 11; values in 0..1 (data range 1).  The definition is
    csrc/ssim.hip's and tests/ssim_numpy.py's: an 11-tap Gaussian window (sigma 1.5) of "valid" extent, biased moments, C1 = 1e-4,
    C2 = 9e-4, every channel on its own, mean over pixels and channels.  There is no luminance conversion and no downsampling:
    this is NOT pyiqa's Y-channel preprocessing, and figures differ from it.  mask [N, H, W] bool: a map pixel counts iff the
    mask is set at its centre (image pixel (i+5, j+5)); an image with no counted pixel gives exactly 1.0 and a zero gradient.
    Gradient goes to x only (y and mask are detached); when x does not require grad nothing is stashed and the result has no
    grad_fn.  Bit-reproducible, and an image's result does not depend on the rest of the batch."""
    what = 'ssim'
    for name, t in (('x', x), ('y', y)):
        if not torch.is_tensor(t):
            raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
        if t.dtype != _F32:
            raise ValueError(f'{what}: {name} must be {_F32}, got {t.dtype}')
        if t.dim() != 4:
            raise ValueError(f'{what}: {name} must be [N, H, W, C], got {tuple(t.shape)}')
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError(f'{what}: x {tuple(x.shape)} and y {tuple(y.shape)}: one shape expected')
    N, H, W, C = x.shape
    if not 1 <= C <= 4:
        raise ValueError(f'{what}: 1 to 4 channels in the last dimension expected, got {tuple(x.shape)}')
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f'{what}: images of at least {SSIM_WINDOW} x {SSIM_WINDOW} expected, got {H} x {W}')
    tensors = [x, y]
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (N, H, W):
            got = f'{tuple(mask.shape)} {mask.dtype}' if torch.is_tensor(mask) else type(mask).__name__
            raise ValueError(f'{what}: mask must be a {torch.bool} tensor [{N}, {H}, {W}] on the GPU, got {got}')
        mask = mask.detach()
        tensors.append(mask)
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: every operand must be contiguous')
    _on_gpu(what, *tensors)
    if any(t.device != x.device for t in tensors):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(t.device) for t in tensors})}')
    if N == 0:
        out = (torch.empty((0,), device=x.device, dtype=_F32),)
        if return_map:
            out += (torch.empty((0, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, C), device=x.device, dtype=_F32),)
        if return_count:
            out += (torch.empty((0,), device=x.device, dtype=_I32),)
        return out[0] if len(out) == 1 else out
    res = _Ssim.apply(x, y.detach(), mask, bool(return_map))
    out = (res[0],) + ((res[2],) if return_map else ()) + ((res[1].detach(),) if return_count else ())
    return out[0] if len(out) == 1 else out


# exemplar-based (PatchMatch) image inpainting (beyond the reference, whose RGB_inpainted/ images are made elsewhere; csrc/exemplar.hip) --

EXEMPLAR_META_HEADER = 96        # int32 words in front of the per-image state (csrc/exemplar.hip: META_STATE)
EXEMPLAR_STATE_WORDS = 32
EXEMPLAR_MAX_LEVELS = 8


def exemplar_fill(images, masks, patch=7, rounds=3, iters=4, seed=0, sources=None, max_levels=None):
    """Fill the masked (and the non-finite) pixels of images [N, H, W, 3] fp32 (0..1) with texture copied from the rest of the
    same image: a pyramid, then nearest-neighbour-field search alternating with voting, coarse to fine, on 8-bit colours in
    integer arithmetic (the definition is csrc/exemplar.hip's and tests/exemplar_numpy.py's; the two agree bit for bit).
    masks [N, H, W] bool; sources [N, H, W] bool restricts the exemplars to patches that lie wholly inside it (None: every known
    pixel); patch: the odd patch side in 3..9; per level `rounds` x (`iters` searches, one vote); max_levels caps the pyramid
    (None: levels are added while min(h, w) // 2 >= 4 patch).  Returns (filled [N, H, W, 3], info).  Outside the hole the output
    is the input bit for bit, inside it is k / 255.  info holds per image numpy arrays `targets`, `sources` (the sizes of the
    two sets at full resolution), `levels` (the levels the image used), `energy` (the summed SSD of the final field, int64),
    `singular` (no exemplar at full resolution: returned unchanged), and the device tensor `nnf` [N, H, W, 2] int32: (y, x) of each
    target's exemplar, -1 off the targets.  The textures are plausible, not pixel-accurate: see DESIGN.md section 18.  One host
    read-back sizes the lists and the per-level launches; info is read after the last launch.  Detached: no autograd."""
    import numpy as np
    what = 'exemplar_fill'
    if not torch.is_tensor(images) or images.dtype != _F32 or images.dim() != 4 or images.shape[-1] != 3:
        got = f'{tuple(images.shape)} {images.dtype}' if torch.is_tensor(images) else type(images).__name__
        raise ValueError(f'{what}: images must be a {_F32} tensor [N, H, W, 3] on the GPU, got {got}')
    v = images.detach()
    m = _image_batch(what, masks, torch.bool, 'masks')
    N, H, W, _ = v.shape
    tensors = [v, m]
    if tuple(m.shape) != (N, H, W):
        raise ValueError(f'{what}: masks {tuple(m.shape)} for images {tuple(v.shape)}: [{N}, {H}, {W}] expected')
    src = None
    if sources is not None:
        src = _image_batch(what, sources, torch.bool, 'sources')
        if tuple(src.shape) != (N, H, W):
            raise ValueError(f'{what}: sources {tuple(src.shape)} for images {tuple(v.shape)}: [{N}, {H}, {W}] expected')
        tensors.append(src)
    patch, rounds, iters, seed = int(patch), int(rounds), int(iters), int(seed)
    if patch % 2 == 0 or not 3 <= patch <= 9:
        raise ValueError(f'{what}: patch must be odd and in 3..9, got {patch}')
    if min(H, W) < patch:
        raise ValueError(f'{what}: images of {H} x {W} are smaller than the patch of {patch}')
    if rounds < 0 or iters < 0:
        raise ValueError(f'{what}: rounds {rounds} and iters {iters} must be >= 0')
    if max_levels is not None and not 1 <= int(max_levels):
        raise ValueError(f'{what}: max_levels must be >= 1 (or None), got {max_levels}')
    if not 0 <= seed < 1 << 32:
        raise ValueError(f'{what}: seed must be in 0 .. 2^32 - 1, got {seed}')
    _on_gpu(what, *tensors)
    if any(t.device != v.device for t in tensors):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(t.device) for t in tensors})}')
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: every operand must be contiguous')
    dev = v.device
    out = torch.empty_like(v)
    nnf = torch.empty((N, H, W, 2), device=dev, dtype=_I32)
    if N == 0:
        e = np.zeros(0, np.int64)
        return out, {'targets': e, 'sources': e.copy(), 'levels': e.copy(), 'energy': e.copy(), 'singular': np.zeros(0, bool), 'nnf': nnf}
    lib = _lib.load()
    L = lib.mvip_exemplar_levels(H, W, patch, 0 if max_levels is None else min(int(max_levels), EXEMPLAR_MAX_LEVELS))
    nbytes = lib.mvip_exemplar_workspace_bytes(N, H, W, patch, L) if L > 0 else -1
    if nbytes < 0:
        raise ValueError(f'{what}: {N} images of {H} x {W} are beyond the kernels\' index range')
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    meta = torch.empty(lib.mvip_exemplar_meta_words(N), device=dev, dtype=_I32)
    st = stream()
    pws, pmeta = ptr(ws, torch.uint8), ptr(meta, _I32)
    call('mvip_exemplar_setup', ptr(v), ptr(m, torch.bool), ptr(src, torch.bool), N, H, W, patch, L, pws, pmeta, st)
    totals = meta[:6 * EXEMPLAR_MAX_LEVELS].cpu().numpy().view(np.int64).reshape(EXEMPLAR_MAX_LEVELS, 3)     # the read-back
    capacity = int(totals.sum())
    lists = torch.empty(max(capacity, 1), device=dev, dtype=_I32)
    call('mvip_exemplar_lists', N, H, W, patch, L, pws, pmeta, ptr(lists, _I32), capacity, st)
    for level in range(L - 1, -1, -1):
        call('mvip_exemplar_level', N, H, W, patch, L, level, int(totals[level, 0]), int(totals[level, 1]), rounds, iters, seed,
             pws, pmeta, ptr(lists, _I32), st)
    call('mvip_exemplar_finish', ptr(v), N, H, W, patch, L, rounds, iters, pws, pmeta, ptr(out), ptr(nnf, _I32), st)
    s = meta[EXEMPLAR_META_HEADER:].cpu().numpy().reshape(N, EXEMPLAR_STATE_WORDS)
    info = {'targets': s[:, 4].astype(np.int64), 'sources': s[:, 6].astype(np.int64), 'levels': s[:, 0].astype(np.int64),
            'energy': np.ascontiguousarray(s[:, 2:4]).view(np.int64).reshape(N).copy(), 'singular': s[:, 1] != 0, 'nnf': nnf}
    return out, info


# mesh clean-up: corner table, vertex normals, Taubin smoothing, vertex clustering (beyond the reference, csrc/mesh_ops.hip) ------
# The definitions are csrc/mesh_ops.hip's and tests/mesh_ops_numpy.py's.  There is no CPU path.

MESH_PLACEMENTS = ('mean', 'quadric')
MAX_CLUSTER_CELLS_PER_AXIS = 512


def _mesh_operands(what, verts, faces, colors=None):
    named = [('verts', verts, _F32), ('faces', faces, _I32)] + ([('colors', colors, torch.uint8)] if colors is not None else [])
    for name, t, dtype in named:
        if not torch.is_tensor(t):
            raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
        if t.dtype != dtype:
            raise ValueError(f'{what}: {name} must be {dtype}, got {t.dtype}')
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f'{what}: {name} must be [{"F" if name == "faces" else "V"}, 3], got {tuple(t.shape)}')
    tensors = [t.detach() for _, t, _ in named]
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(t.device) for t in tensors})}')
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: every operand must be contiguous')
    if colors is not None and colors.shape[0] != verts.shape[0]:
        raise ValueError(f'{what}: colors {tuple(colors.shape)} for verts {tuple(verts.shape)}')
    if verts.shape[0] > 2 ** 31 - 1 or 3 * faces.shape[0] > 2 ** 31 - 1:
        raise ValueError(f'{what}: {verts.shape[0]} vertices / {faces.shape[0]} faces exceed int32 indices')
    return tensors


def _mesh_lists(keys, n_lists):
    """(offsets [n_lists + 1], items [n], flag [1]) of mvip_mesh_corner_table for keys [n] int32; flag is NOT read here."""
    n = int(keys.shape[0])
    dev = keys.device
    if n == 0 or n_lists == 0:
        return (torch.zeros(n_lists + 1, device=dev, dtype=_I32), torch.empty(0, device=dev, dtype=_I32),
                torch.full((1,), 1 if n else 0, device=dev, dtype=_I32))
    words = _lib.load().mvip_mesh_list_scratch_words(n, n_lists)
    if words < 0:
        raise ValueError(f'mesh lists: {n} items in {n_lists} lists exceed int32 indices')
    offsets = torch.empty(n_lists + 1, device=dev, dtype=_I32)
    items = torch.empty(n, device=dev, dtype=_I32)
    scratch = torch.empty(words, device=dev, dtype=_I32)
    flag = torch.empty(1, device=dev, dtype=_I32)
    call('mvip_mesh_corner_table', ptr(keys, _I32), n, n_lists, ptr(offsets, _I32), ptr(items, _I32), ptr(scratch, _I32),
         ptr(flag, _I32), stream())
    return offsets, items, flag


def mesh_corner_table(faces, n_verts):
    """The corner table of faces [F, 3] int32 on the device: (offsets [V + 1] int32, corners [3 F] int32).  Corner c = 3 f + k
    is vertex faces[f, k]; the corners of vertex v are corners[offsets[v]:offsets[v + 1]] in ascending order.  F = 0 or V = 0:
    empty tensors, nothing launched.  ValueError for a face index outside [0, V) (checked on the device, one flag read back:
    the only synchronisation)."""
    what = 'mesh_corner_table'
    n_verts = int(n_verts)
    if n_verts < 0 or n_verts > 2 ** 31 - 2:
        raise ValueError(f'{what}: n_verts must be in 0..2^31 - 2, got {n_verts}')
    if not torch.is_tensor(faces):
        raise ValueError(f'{what}: faces must be a tensor on the GPU, got {type(faces).__name__}')
    if faces.dtype != _I32:
        raise ValueError(f'{what}: faces must be {_I32}, got {faces.dtype}')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f'{what}: faces must be [F, 3], got {tuple(faces.shape)}')
    if not faces.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if not faces.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    if 3 * faces.shape[0] > 2 ** 31 - 1:
        raise ValueError(f'{what}: {faces.shape[0]} faces exceed int32 corner indices')
    F = int(faces.shape[0])
    if F and n_verts == 0:
        raise ValueError(f'{what}: a face index lies outside [0, 0)')
    offsets, corners, flag = _mesh_lists(faces.detach().reshape(-1), n_verts)
    if F and int(flag.cpu()):
        raise ValueError(f'{what}: a face index lies outside [0, {n_verts})')
    return offsets, corners


def mesh_vertex_normals(verts, faces):
    """normals [V, 3] fp32 of an indexed mesh from its faces alone: per vertex the sum over its corner list of
    (p1 - p0) x (p2 - p0) (area-weighted; faces counter-clockwise seen from outside, so it points outward), accumulated in
    fp64, normalised, rounded to fp32; (0, 0, 0) for a vertex without faces or a zero sum."""
    v, f = _mesh_operands('mesh_vertex_normals', verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    offsets, corners = mesh_corner_table(f, V)
    normals = torch.empty((V, 3), device=v.device, dtype=_F32)
    if V:
        call('mvip_mesh_vertex_normals', ptr(v), ptr(f, _I32) if F else ptr(None), V, F, ptr(offsets, _I32),
             ptr(corners, _I32) if F else ptr(None), ptr(normals), stream())
    return normals


def mesh_smooth(verts, faces, iters=10, lam=0.5, mu=-0.53):
    """Taubin smoothing: new verts [V, 3] fp32.  One iteration is two gather passes, v <- v + lam L(v) then v <- v + mu L(v),
    L(v) = (sum over v's corners of (a + b)) / (2 n_corners) - v with a, b the other two vertices of the corner's face (on a
    closed manifold the uniform umbrella: every neighbour is in exactly two incident faces), summed in fp64 in corner order;
    a pass reads only the previous pass's positions (two buffers in turn) and vertices without faces do not move.  The
    corner table is built once.  ValueError for iters < 0, non-finite lam or mu, lam <= 0, mu >= 0, mu > -lam.  iters = 0: a
    copy."""
    import math
    what = 'mesh_smooth'
    v, f = _mesh_operands(what, verts, faces)
    if int(iters) != iters or int(iters) < 0:
        raise ValueError(f'{what}: iters must be an integer >= 0, got {iters!r}')
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)) or lam <= 0 or mu >= 0 or mu > -lam:
        raise ValueError(f'{what}: lam {lam} and mu {mu} must be finite with lam > 0 and mu <= -lam < 0')
    V, F = int(v.shape[0]), int(f.shape[0])
    cur = v.clone()
    if int(iters) == 0 or V == 0:
        return cur
    offsets, corners = mesh_corner_table(f, V)
    if F == 0:
        return cur
    nxt = torch.empty_like(cur)
    for _ in range(int(iters)):
        for w in (lam, mu):
            call('mvip_mesh_smooth_pass', ptr(cur), ptr(f, _I32), V, F, ptr(offsets, _I32), ptr(corners, _I32), w, ptr(nxt), stream())
            cur, nxt = nxt, cur
    return cur


def mesh_cluster_grid(lo, hi, cell, origin=None):
    """The clustering lattice of mesh_cluster for vertices whose componentwise minimum / maximum are lo / hi (fp32 [3]):
    (origin fp32 [3], inv fp32, cells (cx, cy, cz)).  origin defaults to lo; inv = fp32(1 / cell); the count of an axis is
    floor(extent / cell) + 1 evaluated by the cell rule itself, floorf(fp32(hi - origin) * inv) + 1 in fp32, so the largest
    vertex is in the last cell whatever the rounding.  ValueError for a cell that is not finite and > 0, non-finite
    vertices or origin, a vertex below the origin, an axis of more than 512 cells (the message names the smallest
    admissible cell)."""
    import math
    import numpy as np
    what = 'mesh_cluster'
    cell = float(cell)
    if not (math.isfinite(cell) and cell > 0):
        raise ValueError(f'{what}: cell must be finite and > 0, got {cell}')
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError(f'{what}: a vertex is NaN or infinite')
    o = lo if origin is None else np.asarray([float(x) for x in origin], np.float32)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError(f'{what}: origin must be three finite coordinates, got {origin!r}')
    with np.errstate(over='ignore', divide='ignore'):
        inv = np.float32(1.0 / cell)
        n = np.floor((hi - o).astype(np.float32) * inv)
    if not (math.isfinite(float(inv)) and inv > 0):
        raise ValueError(f'{what}: 1 / cell is not a finite fp32 number > 0 for cell {cell}')
    if np.any(lo < o) or np.any(n < 0):
        raise ValueError(f'{what}: a vertex lies outside the box that starts at origin {o.tolist()}')
    if np.any(n + 1 > MAX_CLUSTER_CELLS_PER_AXIS):
        need = float(np.max(hi.astype(np.float64) - o.astype(np.float64))) / MAX_CLUSTER_CELLS_PER_AXIS
        raise ValueError(f'{what}: cell {cell} gives {[int(x) + 1 for x in n]} cells, at most {MAX_CLUSTER_CELLS_PER_AXIS} per axis: '
                         f'the smallest admissible cell is just above {need:.9g}')
    return o, inv, tuple(int(x) + 1 for x in n)


def mesh_cluster(verts, faces, colors, origin, cell, placement='quadric', dedupe=False):
    """Simplification by vertex clustering (the definition: csrc/mesh_ops.hip, tests/mesh_ops_numpy.py): returns
    (verts' [V', 3] fp32, faces' [F', 3] int32, colors' uint8 [V', 3] or None, cluster_of_vertex [V] int32: the new vertex of
    each input vertex, -1 for the vertices of dropped clusters).

    The clusters are the occupied cells of a bit grid (bitgrid.py) that starts at `origin` (None: the componentwise minimum of
    the vertices) with cubic cells of edge `cell`, 1..512 per axis; ids ascend in (ix, iy, iz), z fastest.  placement 'mean':
    the mean of the members; 'quadric': the minimiser of the summed squared distances to the area-weighted planes of the
    cluster's corners, falling back to the mean when the system is near-singular or the minimiser leaves the cluster's own
    cell -- so no vertex moves by more than sqrt(3) cell.  colors (uint8 [V, 3] or None): exact integer means.  Faces are
    remapped, those with two equal ids dropped, the rest kept in input order; clusters that no surviving face references are
    dropped and the rest renumbered in order.

    dedupe=False is the default for a reason: a closed input (every directed edge (a, b) as often as (b, a)) stays closed,
    because a collapsed face contributes (a, a), (a, b), (b, a), which cancel.  dedupe=True also drops every face whose
    directed cycle, up to rotation, occurred earlier (the opposite orientation is a different face); removing duplicates can
    break that balance.  ValueError for a vertex outside the box, NaN or infinite, a face index outside [0, V), more than 512
    cells on an axis.  Reads back the vertex bounds, the cluster count and the two output sizes."""
    import ctypes
    import numpy as np
    what = 'mesh_cluster'
    v, f, *c = _mesh_operands(what, verts, faces, colors)
    c = c[0] if c else None
    if placement not in MESH_PLACEMENTS:
        raise ValueError(f"{what}: placement must be 'mean' or 'quadric', got {placement!r}")
    V, F = int(v.shape[0]), int(f.shape[0])
    dev = v.device
    if V == 0:
        if F:
            raise ValueError(f'{what}: a face index lies outside [0, 0)')
        mesh_cluster_grid((0, 0, 0), (0, 0, 0), cell, origin)
        return (torch.empty((0, 3), device=dev, dtype=_F32), torch.empty((0, 3), device=dev, dtype=_I32),
                None if c is None else torch.empty((0, 3), device=dev, dtype=torch.uint8), torch.empty(0, device=dev, dtype=_I32))
    lohi = torch.stack([v.amin(0), v.amax(0)]).cpu().numpy()
    o, inv, cells = mesh_cluster_grid(lohi[0], lohi[1], cell, origin)
    cbox = (ctypes.c_float * 6)(*([float(x) for x in o] + [float(inv)] * 3))
    ccells = (ctypes.c_int * 3)(*cells)
    lib = _lib.load()
    st = stream()
    nw = occupancy_words(cells)
    words = torch.empty(nw, device=dev, dtype=_I32)
    word_rank = torch.empty(nw, device=dev, dtype=_I32)
    wg = torch.empty(max(1, lib.mvip_mesh_rank_groups(nw)), device=dev, dtype=_I32)
    cellv = torch.empty(V, device=dev, dtype=_I32)
    cov = torch.empty(V, device=dev, dtype=_I32)
    meta = torch.empty(2, device=dev, dtype=torch.int64)                     # [0] the cluster count, [1] (low word) the flag
    call('mvip_mesh_cluster_assign', ptr(v), V, cbox, ccells, ptr(words, _I32), ptr(cellv, _I32), ptr(word_rank, _I32),
         ptr(wg, _I32), ptr(meta, torch.int64), ptr(cov, _I32), ctypes.c_void_p(meta.data_ptr() + 8), st)
    K, outside = (int(x) for x in meta.cpu().numpy().view(np.int32)[[0, 2]])
    if outside:
        raise ValueError(f'{what}: a vertex lies outside the box that starts at origin {o.tolist()}, or is NaN or infinite')
    rf = torch.empty(3 * F, device=dev, dtype=_I32)
    if F:
        call('mvip_mesh_gather', ptr(f, _I32), 3 * F, ptr(cov, _I32), V, ptr(rf, _I32), st)
    mem_off, mem, _ = _mesh_lists(cov, K)
    cor_off, cor, bad = _mesh_lists(rf, K)
    if F and int(bad.cpu()):
        raise ValueError(f'{what}: a face index lies outside [0, {V})')
    rep = torch.empty((K, 3), device=dev, dtype=_F32)
    repc = None if c is None else torch.empty((K, 3), device=dev, dtype=torch.uint8)
    none = ptr(None)
    call('mvip_mesh_cluster_place', ptr(v), ptr(c, torch.uint8), ptr(f, _I32) if F else none, V, F, cbox, ccells, float(cell), K,
         ptr(mem_off, _I32), ptr(mem, _I32), ptr(cor_off, _I32), ptr(cor, _I32) if F else none, ptr(cellv, _I32),
         MESH_PLACEMENTS.index(placement), ptr(rep), ptr(repc, torch.uint8), st)
    keep = torch.empty(F, device=dev, dtype=_I32)
    frank = torch.empty(F, device=dev, dtype=_I32)
    fwg = torch.empty(max(1, lib.mvip_mesh_rank_groups(F)), device=dev, dtype=_I32)
    ref = torch.empty(K, device=dev, dtype=_I32)
    crank = torch.empty(K, device=dev, dtype=_I32)
    cwg = torch.empty(max(1, lib.mvip_mesh_rank_groups(K)), device=dev, dtype=_I32)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    pf = (lambda t: ptr(t, _I32) if F else none)
    call('mvip_mesh_cluster_faces', pf(rf), F, K, ptr(cor_off, _I32), pf(cor), int(bool(dedupe)), pf(keep), ptr(ref, _I32),
         ptr(fwg, _I32), pf(frank), ptr(cwg, _I32), ptr(crank, _I32), ptr(totals, torch.int64), st)
    F2, V2 = (int(x) for x in totals.cpu())
    out_v = torch.empty((V2, 3), device=dev, dtype=_F32)
    out_c = None if c is None else torch.empty((V2, 3), device=dev, dtype=torch.uint8)
    out_f = torch.empty((F2, 3), device=dev, dtype=_I32)
    call('mvip_mesh_cluster_emit', pf(rf), F, pf(keep), pf(frank), ptr(rep), ptr(repc, torch.uint8), K, ptr(ref, _I32),
         ptr(crank, _I32), V, F2, V2, ptr(cov, _I32), ptr(out_v) if V2 else none, ptr(out_c, torch.uint8) if V2 else none,
         ptr(out_f, _I32) if F2 else none, st)
    return out_v, out_f, out_c, cov


# mesh topology: edge table, face components, boundary loops, hole caps (beyond the reference, csrc/mesh_topology.hip) ---------
# The definitions are csrc/mesh_topology.hip's and tests/mesh_topology_numpy.py's.  There is no CPU path.

MESH_CONNECTIVITIES = ('edge', 'vertex')
MeshEdgeTable = collections.namedtuple('MeshEdgeTable', 'edge_of edges first count forward twin')
MeshBoundaryLoops = collections.namedtuple('MeshBoundaryLoops', 'loop_of next first sizes closed')


def _topology_faces(what, faces, n_verts):
    n_verts = int(n_verts)
    if n_verts < 0 or n_verts > 2 ** 31 - 2:
        raise ValueError(f'{what}: n_verts must be in 0..2^31 - 2, got {n_verts}')
    if not torch.is_tensor(faces):
        raise ValueError(f'{what}: faces must be a tensor on the GPU, got {type(faces).__name__}')
    if faces.dtype != _I32:
        raise ValueError(f'{what}: faces must be {_I32}, got {faces.dtype}')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f'{what}: faces must be [F, 3], got {tuple(faces.shape)}')
    if not faces.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if not faces.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    if 3 * faces.shape[0] > 2 ** 31 - 1:
        raise ValueError(f'{what}: {faces.shape[0]} faces exceed int32 half-edge indices')
    if faces.shape[0] and n_verts == 0:
        raise ValueError(f'{what}: a face index lies outside [0, 0)')
    return faces.detach(), n_verts


def _rank_wg(n, dev):
    return torch.empty(max(1, _lib.load().mvip_mesh_rank_groups(n)), device=dev, dtype=_I32)


class _HalfEdges:
    """The per-half-edge state every topology op starts from (F > 0): rep, hcount, hforward, twin, rank [3F] and E."""

    def __init__(self, what, f, V):
        F = int(f.shape[0])
        dev = f.device
        n = 3 * F
        st = stream()
        i32 = lambda *shape: torch.empty(shape, device=dev, dtype=_I32)
        keys, flag = i32(n), i32(1)
        call('mvip_mesh_topology_keys', ptr(f, _I32), F, V, ptr(keys, _I32), ptr(flag, _I32), st)
        offsets, items, _ = _mesh_lists(keys, V)          # the lists' own flag only says that some key is -1
        self.rep, self.hcount, self.hforward, self.twin, self.rank = i32(n), i32(n), i32(n), i32(n), i32(n)
        meta = torch.empty(1, device=dev, dtype=torch.int64)
        p = lambda t: ptr(t, _I32)
        call('mvip_mesh_topology_edges_find', p(f), F, V, p(keys), p(offsets), p(items), p(self.rep), p(self.hcount),
             p(self.hforward), p(self.twin), p(_rank_wg(n, dev)), p(self.rank), ptr(meta, torch.int64), st)
        if int(flag.cpu()):
            raise ValueError(f'{what}: a face index lies outside [0, {V})')
        self.E = int(meta.cpu())
        self.f, self.F, self.V = f, F, V

    def edge_table(self):
        dev, E, n = self.f.device, self.E, 3 * self.F
        i32 = lambda *shape: torch.empty(shape, device=dev, dtype=_I32)
        edge_of, edges, first, count, forward = i32(n), i32(E, 2), i32(E), i32(E), i32(E)
        p = lambda t: ptr(t, _I32) if t.numel() else ptr(None)
        call('mvip_mesh_topology_edges_emit', p(self.f), self.F, p(self.rep), p(self.hcount), p(self.hforward), p(self.rank), E,
             p(edge_of), p(edges), p(first), p(count), p(forward), stream())
        return MeshEdgeTable(edge_of, edges, first, count, forward, self.twin)


def _empty_i32(dev, *shape):
    return torch.empty(shape, device=dev, dtype=_I32)


def mesh_edge_table(faces, n_verts):
    """The edge table of faces [F, 3] int32 on the device (csrc/mesh_topology.hip): MeshEdgeTable(edge_of [3F], edges [E, 2] =
    (lo, hi), first [E], count [E], forward [E], twin [3F]), all int32.  Half-edge h = 3 f + k runs from faces[f, k] to
    faces[f, (k + 1) % 3]; an edge is the set of half-edges with the same unordered endpoints; edges are numbered by their
    lowest half-edge `first`; count = its half-edges, forward = those that run lo -> hi; twin = the other half-edge of an edge
    with exactly two, else -1.  count 1: boundary; 2 with forward 1: interior; 2 otherwise: inconsistently oriented; >= 3:
    non-manifold.  A face that names a vertex twice has edge_of = twin = -1.  F = 0 or V = 0: empty tensors, nothing
    launched.  ValueError for a face index outside [0, V).  Reads back the flag and E."""
    what = 'mesh_edge_table'
    f, V = _topology_faces(what, faces, n_verts)
    if f.shape[0] == 0:
        e = lambda *s: _empty_i32(f.device, *s)
        return MeshEdgeTable(e(0), e(0, 2), e(0), e(0), e(0), e(0))
    return _HalfEdges(what, f, V).edge_table()


def _mesh_components(what, he, connectivity):
    f, F, V = he.f, he.F, he.V
    dev = f.device
    st = stream()
    p = lambda t: ptr(t, _I32) if t.numel() else ptr(None)
    offsets, corners = mesh_corner_table(f, V)
    parent, is_root, rank = _empty_i32(dev, F), _empty_i32(dev, F), _empty_i32(dev, F)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    call('mvip_mesh_topology_components_label', p(f), F, V, MESH_CONNECTIVITIES.index(connectivity), p(he.rep), p(offsets),
         p(corners), p(parent), p(is_root), p(_rank_wg(F, dev)), p(rank), ptr(total, torch.int64), st)
    C = int(total.cpu())
    labels, table = _empty_i32(dev, F), _empty_i32(dev, C, 6)
    call('mvip_mesh_topology_components_emit', p(f), F, V, p(parent), p(rank), C, p(he.rep), p(he.hcount), p(he.hforward),
         p(offsets), p(corners), p(labels), p(table), st)
    return labels, table


def mesh_components(faces, n_verts, connectivity='edge'):
    """Connected components of the faces [F, 3] int32 of a mesh: (labels [F] int32, table [C, 6] int32).  connectivity 'edge':
    two faces that share an edge (unordered endpoints) are connected; 'vertex': two faces that share a vertex.  labels are
    1..C in order of each component's lowest face index (ops.grid_components' convention), 0 for a face that names a vertex
    twice.  table columns: faces, vertices, edges, boundary edges (one face), non-manifold edges (three or more), inconsistently
    oriented edges (two faces that run it the same way); V - E + F of a component is table[:, 1] - table[:, 2] + table[:, 0].
    F = 0 or V = 0: empty tensors, nothing launched.  ValueError for another connectivity or a face index outside [0, V)."""
    what = 'mesh_components'
    if connectivity not in MESH_CONNECTIVITIES:
        raise ValueError(f"{what}: connectivity must be 'edge' or 'vertex', got {connectivity!r}")
    f, V = _topology_faces(what, faces, n_verts)
    if f.shape[0] == 0:
        return _empty_i32(f.device, 0), _empty_i32(f.device, 0, 6)
    return _mesh_components(what, _HalfEdges(what, f, V), connectivity)


def _mesh_boundary_loops(he):
    f, F, V = he.f, he.F, he.V
    dev = f.device
    n = 3 * F
    st = stream()
    p = lambda t: ptr(t, _I32) if t.numel() else ptr(None)
    offsets, corners = mesh_corner_table(f, V)
    ends, nxt, parent, is_root, rank = (_empty_i32(dev, V), _empty_i32(dev, n), _empty_i32(dev, n), _empty_i32(dev, n),
                                        _empty_i32(dev, n))
    total = torch.empty(1, device=dev, dtype=torch.int64)
    call('mvip_mesh_topology_loops_label', p(f), F, V, p(he.rep), p(he.hcount), p(offsets), p(corners), p(ends), p(nxt), p(parent),
         p(is_root), p(_rank_wg(n, dev)), p(rank), ptr(total, torch.int64), st)
    L = int(total.cpu())
    loop_of, first, sizes, closed = _empty_i32(dev, n), _empty_i32(dev, L), _empty_i32(dev, L), _empty_i32(dev, L)
    call('mvip_mesh_topology_loops_emit', F, p(parent), p(rank), p(nxt), L, p(loop_of), p(first), p(sizes), p(closed), st)
    return MeshBoundaryLoops(loop_of, nxt, first, sizes, closed)


def mesh_boundary_loops(faces, n_verts):
    """The boundary loops of faces [F, 3] int32: MeshBoundaryLoops(loop_of [3F], next [3F], first [L], sizes [L], closed [L]),
    all int32.  A boundary half-edge is the only half-edge of its edge.  next[h] of a boundary half-edge a -> b is the boundary
    half-edge that starts at b if exactly one starts and exactly one ends there, else -1 (a pinch vertex, where the walk is
    ambiguous); -1 for every other half-edge.  Loops are the chains of next, numbered by their lowest half-edge `first`;
    loop_of is -1 off the boundary; closed[l] = 1 iff every member has a next, and such a loop is a simple cycle.  F = 0 or
    V = 0: empty tensors, nothing launched.  ValueError for a face index outside [0, V)."""
    what = 'mesh_boundary_loops'
    f, V = _topology_faces(what, faces, n_verts)
    if f.shape[0] == 0:
        e = lambda *s: _empty_i32(f.device, *s)
        return MeshBoundaryLoops(e(0), e(0), e(0), e(0), e(0))
    return _mesh_boundary_loops(_HalfEdges(what, f, V))


def mesh_cap_loops(verts, faces, colors, max_edges):
    """Centroid-fan caps of the small boundary loops of a mesh: (new_verts [N, 3] fp32, new_colors uint8 [N, 3] or None,
    new_faces [M, 3] int32, capped [L] int32).  A loop of mesh_boundary_loops is capped iff it is closed and has 3..max_edges
    half-edges.  Per capped loop one new vertex, the mean of the loop's origin vertices (fp64 sum in ascending half-edge
    order, rounded to fp32 once; colours: exact integer means), numbered V, V + 1, ... in loop order; per boundary half-edge
    a -> b of it the face (b, a, new vertex), in ascending half-edge order: reversed, so a consistently oriented mesh stays
    consistent.  The capped mesh is cat(verts, new_verts), cat(faces, new_faces).  F = 0 or V = 0: empty tensors, nothing
    launched.  ValueError for max_edges < 3 or a face index outside [0, V)."""
    what = 'mesh_cap_loops'
    v, f, *c = _mesh_operands(what, verts, faces, colors)
    c = c[0] if c else None
    if int(max_edges) != max_edges or int(max_edges) < 3:
        raise ValueError(f'{what}: max_edges must be an integer >= 3, got {max_edges!r}')
    max_edges = min(int(max_edges), 2 ** 31 - 1)
    f, V = _topology_faces(what, f, v.shape[0])
    dev = v.device
    F = int(f.shape[0])
    none_c = None if c is None else torch.empty((0, 3), device=dev, dtype=torch.uint8)
    if F == 0:
        return torch.empty((0, 3), device=dev, dtype=_F32), none_c, _empty_i32(dev, 0, 3), _empty_i32(dev, 0)
    loops = _mesh_boundary_loops(_HalfEdges(what, f, V))
    L, n = int(loops.first.shape[0]), 3 * F
    st = stream()
    p = lambda t: ptr(t, _I32) if t.numel() else ptr(None)
    capped, keys, loop_rank, he_rank = _empty_i32(dev, L), _empty_i32(dev, n), _empty_i32(dev, L), _empty_i32(dev, n)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    call('mvip_mesh_topology_cap_plan', F, p(loops.loop_of), L, p(loops.sizes), p(loops.closed), max_edges, p(capped), p(keys),
         p(_rank_wg(L, dev)), p(loop_rank), p(_rank_wg(n, dev)), p(he_rank), ptr(totals, torch.int64), st)
    n_caps, n_cap_faces = (int(x) for x in totals.cpu())
    new_v = torch.empty((n_caps, 3), device=dev, dtype=_F32)
    new_c = None if c is None else torch.empty((n_caps, 3), device=dev, dtype=torch.uint8)
    new_f = _empty_i32(dev, n_cap_faces, 3)
    if n_caps:
        loop_off, loop_items, _ = _mesh_lists(keys, L)
        call('mvip_mesh_topology_cap_emit', ptr(v), ptr(c, torch.uint8), p(f), V, F, L, p(keys), p(capped), p(loop_rank), p(he_rank),
             p(loop_off), p(loop_items), n_caps, n_cap_faces, ptr(new_v), ptr(new_c, torch.uint8), p(new_f), st)
    return new_v, new_c, new_f, capped


# mesh-to-mesh distance: closest-point queries on a grid of face lists, surface samples (beyond the reference, csrc/mesh_distance.hip)
# The definition is csrc/mesh_distance.hip's and tests/mesh_distance_numpy.py's.  There is no CPU path.

FACE_GRID_MAX_CELLS_PER_AXIS = 512
# a cell is never narrower than this share of the largest coordinate magnitude (the margin argument of csrc/mesh_distance.hip)
FACE_GRID_MIN_CELL_SHARE = 2.0 ** -20
MESH_SAMPLE_MAX_SUBDIVISION = 1024


class FaceGrid:
    """The face lists of one mesh on a uniform grid (ops.mesh_face_grid): reusable for any number of mesh_closest_point calls
    on the same verts / faces tensors.  box = (bmin[3], inv[3]) fp32, cells (cx, cy, cz), cell_offsets [n_cells + 1] int32,
    cell_faces [n_pairs] int32 (each cell's faces ascending), n_pairs; bounds = the fp32 (minimum[3], maximum[3]) of the vertices
    as a host array [6] (what the ray casts of csrc/mesh_raycast.hip cut their rays to)."""

    def __init__(self, verts, faces, box, cells, cell_offsets, cell_faces, bounds=None):
        self.verts, self.faces, self.box, self.cells = verts, faces, box, cells
        self.cell_offsets, self.cell_faces = cell_offsets, cell_faces
        self.n_pairs = int(cell_faces.shape[0])
        self.bounds = bounds
        self._key = self._key_of(verts, faces)

    @staticmethod
    def _key_of(v, f):
        return (v.data_ptr(), tuple(v.shape), v._version, f.data_ptr(), tuple(f.shape), f._version, str(v.device))

    def matches(self, verts, faces):
        return self._key == self._key_of(verts, faces)


def mesh_face_grid_cells(lo, hi, n_faces, cells=None):
    """(box fp32 [6] = (bmin, inv), cells (cx, cy, cz)) of the face grid over the bounding box lo .. hi (fp32 [3]) of a mesh of
    n_faces faces.  Host code.  Default: cubic cells of edge h = (the product of the non-zero extents / n_faces)^(1 / their number),
    about one cell per face; ceil(extent / h) cells per axis clamped to 1..512, inv = fp32(1 / h) on all axes.  cells (an int or
    three): that many per axis, inv = fp32(cells / extent) per axis.  An axis of zero extent has one cell and inv 1.  Every count
    is then cut down so that no cell is narrower than 2^-20 of the largest coordinate magnitude (never on a sane mesh).
    ValueError for non-finite bounds or counts outside 1..512."""
    import math
    import numpy as np
    what = 'mesh_face_grid'
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError(f'{what}: a vertex is NaN or infinite')
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    if not np.all(np.isfinite(ext.astype(np.float32))) or np.any(ext < 0):
        raise ValueError(f'{what}: the bounding box {lo.tolist()} .. {hi.tolist()} has no finite fp32 extent')
    scale = float(max(np.abs(lo).max(), np.abs(hi).max()))
    narrowest = scale * FACE_GRID_MIN_CELL_SHARE
    cap = [FACE_GRID_MAX_CELLS_PER_AXIS if narrowest == 0 else int(max(1, min(FACE_GRID_MAX_CELLS_PER_AXIS, math.floor(e / narrowest))))
           for e in ext]
    if cells is None:
        nz = [e for e in ext if e > 0]
        if not nz:
            counts, h = [1, 1, 1], 1.0
        else:
            h = (float(np.prod(nz)) / max(int(n_faces), 1)) ** (1.0 / len(nz))
            counts = [1 if e == 0 else int(max(1, min(cap[a], math.ceil(e / h * (1.0 - 1e-12))))) for a, e in enumerate(ext)]
            h = max(h, max(e / c for e, c in zip(ext, counts)))                  # clamped counts: the cells grow, still cubic
        inv = [np.float32(1.0) if e == 0 else np.float32(1.0 / h) for e in ext]
    else:
        counts = [int(cells)] * 3 if np.isscalar(cells) else [int(c) for c in cells]
        if len(counts) != 3 or not all(1 <= c <= FACE_GRID_MAX_CELLS_PER_AXIS for c in counts):
            raise ValueError(f'{what}: cells must be one or three counts in 1..{FACE_GRID_MAX_CELLS_PER_AXIS}, got {cells!r}')
        counts = [1 if e == 0 else min(c, cap[a]) for a, (e, c) in enumerate(zip(ext, counts))]
        inv = [np.float32(1.0) if e == 0 else np.float32(c / e) for e, c in zip(ext, counts)]
    if not all(math.isfinite(float(i)) and i > 0 for i in inv):
        raise ValueError(f'{what}: 1 / cell is not a finite fp32 number > 0 for the box {lo.tolist()} .. {hi.tolist()}')
    return np.concatenate([lo, np.asarray(inv, np.float32)]).astype(np.float32), tuple(counts)


def mesh_face_grid(verts, faces, cells=None):
    """The reusable FaceGrid of an indexed mesh for mesh_closest_point (the definition: csrc/mesh_distance.hip): a uniform grid
    over the mesh's bounding box (mesh_face_grid_cells: about one cubic cell per face by default, `cells` = an int or three counts
    for the tests) with every face entered in every cell its bounding box overlaps, each cell's list ascending in the face index.
    Built from per-face counts, an exclusive scan, the (cell, face) pairs in face order and the lists of mesh_corner_table over
    the cell keys.  ValueError for F = 0, a face index outside [0, V), a NaN or infinite vertex, more than 2^31 - 1 pairs.  Reads
    back the vertex bounds, then the pair total with the flag."""
    import ctypes
    import numpy as np
    what = 'mesh_face_grid'
    v, f = _mesh_operands(what, verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0 or V == 0:
        raise ValueError(f'{what}: a mesh of {F} faces and {V} vertices has no closest point')
    dev = v.device
    lohi = torch.stack([v.amin(0), v.amax(0)]).cpu().numpy()
    box, counts = mesh_face_grid_cells(lohi[0], lohi[1], F, cells)
    cbox = (ctypes.c_float * 6)(*[float(x) for x in box])
    ccells = (ctypes.c_int * 3)(*counts)
    st = stream()
    face_off = torch.empty(F, device=dev, dtype=torch.int64)
    meta = torch.empty(2, device=dev, dtype=torch.int64)                     # [0] the pair total, [1] (low word) the flag
    call('mvip_mesh_distance_grid_count', ptr(v), ptr(f, _I32), V, F, cbox, ccells, ptr(face_off, torch.int64), ptr(meta, torch.int64),
         ctypes.c_void_p(meta.data_ptr() + 8), st)
    host = meta.cpu().numpy()
    P, flag = int(host[0]), int(host.view(np.int32)[2])
    if flag & 1:
        raise ValueError(f'{what}: a face index lies outside [0, {V})')
    if flag & 2:
        raise ValueError(f'{what}: a vertex is NaN or infinite')
    words = _lib.load().mvip_mesh_distance_grid_scratch_words(P, ccells)
    if P > 2 ** 31 - 1 or words < 0:
        raise ValueError(f'{what}: {P} (cell, face) pairs on {counts} cells exceed int32 indices: use fewer cells')
    K = counts[0] * counts[1] * counts[2]
    cell_off = torch.empty(K + 1, device=dev, dtype=_I32)
    cell_faces = torch.empty(P, device=dev, dtype=_I32)
    scratch = torch.empty(words, device=dev, dtype=_I32)
    call('mvip_mesh_distance_grid_fill', ptr(v), ptr(f, _I32), V, F, cbox, ccells, ptr(face_off, torch.int64), P, ptr(cell_off, _I32),
         ptr(cell_faces, _I32), ptr(scratch, _I32), st)
    return FaceGrid(v, f, box, counts, cell_off, cell_faces, bounds=lohi.reshape(6).astype(np.float32))


def mesh_closest_point(points, verts, faces, grid=None, return_stats=False):
    """The closest point of the mesh (verts [V, 3] fp32, faces [F, 3] int32) to each of points [N, 3] fp32, all on the GPU:
    (face [N] int32, point [N, 3] fp32, dist [N] fp32).  The definition (csrc/mesh_distance.hip, tests/mesh_distance_numpy.py):
    per face the exact point-triangle distance in fp64 on the widened inputs, a degenerate face being its edges; the face of
    smallest squared distance, the lowest index among equals; point and dist rounded to fp32 once.  A query with a NaN or
    infinite coordinate gives face -1 and NaN.  grid: a FaceGrid of mesh_face_grid for these very tensors (None: built here);
    the result does not depend on it.  return_stats=True appends a [2] int64 device tensor (a counting variant of the kernel):
    the number of point-face tests and, summed over the waves, 64 times the tests of the wave's busiest lane.  N = 0 gives empty tensors.  ValueError for bad shapes or dtypes, CPU tensors, F = 0, a
    face index outside [0, V), a NaN or infinite vertex, a grid of another mesh.  Detached."""
    import ctypes
    what = 'mesh_closest_point'
    v, f = _mesh_operands(what, verts, faces)
    if not torch.is_tensor(points):
        raise ValueError(f'{what}: points must be a tensor on the GPU, got {type(points).__name__}')
    if points.dtype != _F32:
        raise ValueError(f'{what}: points must be {_F32}, got {points.dtype}')
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'{what}: points must be [N, 3], got {tuple(points.shape)}')
    p = points.detach()
    if not p.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if p.device != v.device:
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(v.device), str(p.device)})}')
    if not p.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    N = int(p.shape[0])
    if 3 * N > 2 ** 31 - 1:
        raise ValueError(f'{what}: {N} points exceed int32 indices')
    if grid is None:
        grid = mesh_face_grid(v, f)
    elif not isinstance(grid, FaceGrid) or not grid.matches(v, f):
        raise ValueError(f'{what}: grid must be the mesh_face_grid of these verts and faces')
    V, F = int(v.shape[0]), int(f.shape[0])
    dev = v.device
    face = torch.empty(N, device=dev, dtype=_I32)
    point = torch.empty((N, 3), device=dev, dtype=_F32)
    dist = torch.empty(N, device=dev, dtype=_F32)
    stats = torch.empty(2, device=dev, dtype=torch.int64) if return_stats else None
    none = ptr(None)
    cbox = (ctypes.c_float * 6)(*[float(x) for x in grid.box])
    ccells = (ctypes.c_int * 3)(*grid.cells)
    call('mvip_mesh_distance_query', ptr(p) if N else none, N, ptr(v), ptr(f, _I32), V, F, cbox, ccells, ptr(grid.cell_offsets, _I32),
         ptr(grid.cell_faces, _I32) if grid.n_pairs else none, grid.n_pairs, ptr(face, _I32) if N else none, ptr(point) if N else none,
         ptr(dist) if N else none, ptr(stats, torch.int64) if return_stats else none, stream())
    return (face, point, dist, stats) if return_stats else (face, point, dist)


def mesh_sample_faces(verts, faces, k):
    """Deterministic surface samples: (points [F k^2, 3] fp32, face_of_sample [F k^2] int32, weights [F k^2] fp64), face-major.
    The k^2 centroids of the uniform subdivision of each face into k^2 congruent triangles (upward ones first, then downward;
    csrc/mesh_distance.hip), each carrying area(face) / k^2: an exact equal-area quadrature rule, nothing random.  fp64
    arithmetic, points rounded to fp32.  F = 0 gives empty tensors.  ValueError for k outside 1..1024, more than 2^31 - 1
    coordinates, a face index outside [0, V)."""
    what = 'mesh_sample_faces'
    v, f = _mesh_operands(what, verts, faces)
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MESH_SAMPLE_MAX_SUBDIVISION:
        raise ValueError(f'{what}: k must be an integer in 1..{MESH_SAMPLE_MAX_SUBDIVISION}, got {k!r}')
    k = int(k)
    V, F = int(v.shape[0]), int(f.shape[0])
    n = F * k * k
    if 3 * n > 2 ** 31 - 1:
        raise ValueError(f'{what}: {n} samples exceed int32 indices')
    if F and V == 0:
        raise ValueError(f'{what}: a face index lies outside [0, 0)')
    dev = v.device
    pts = torch.empty((n, 3), device=dev, dtype=_F32)
    fos = torch.empty(n, device=dev, dtype=_I32)
    w = torch.empty(n, device=dev, dtype=torch.float64)
    flag = torch.empty(1, device=dev, dtype=_I32)
    none = ptr(None)
    call('mvip_mesh_sample_faces', ptr(v) if V else none, ptr(f, _I32) if F else none, V, F, k, ptr(pts) if n else none,
         ptr(fos, _I32) if n else none, ptr(w, torch.float64) if n else none, ptr(flag, _I32), stream())
    if int(flag.cpu()):
        raise ValueError(f'{what}: a face index lies outside [0, {V})')
    return pts, fos, w


# signed mesh distance: pseudonormal sign on the closest point, for points or a lattice (beyond the reference, csrc/mesh_sdf.hip) ---
# The definition is csrc/mesh_sdf.hip's and tests/mesh_sdf_numpy.py's.  There is no CPU path.

def mesh_vertex_pseudonormals(verts, faces):
    """P [V, 3] fp64 of an indexed mesh: per vertex the sum over its corner list, in order, of (the angle of the corner) x (the
    unit normal of its face), in fp64, unnormalised; zeros for a vertex without faces (csrc/mesh_sdf.hip).  The sign of
    mesh_signed_distance at a query whose closest point is a vertex.  ValueError as mesh_corner_table."""
    v, f = _mesh_operands('mesh_vertex_pseudonormals', verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    offsets, corners = mesh_corner_table(f, V)
    P = torch.empty((V, 3), device=v.device, dtype=torch.float64)
    if V:
        call('mvip_mesh_vertex_pseudonormals', ptr(v), ptr(f, _I32) if F else ptr(None), V, F, ptr(offsets, _I32),
             ptr(corners, _I32) if F else ptr(None), ptr(P, torch.float64), stream())
    return P


def _band(what, max_dist):
    if max_dist is None:
        return float('inf')
    B = float(max_dist)
    if not B >= 0.0:
        raise ValueError(f'{what}: max_dist must be None or a number >= 0, got {max_dist!r}')
    return B


def _sdf_mesh(what, verts, faces, grid, twin, pseudonormals):
    """The mesh operands of mvip_mesh_signed_distance, checked; whatever is not given is built here."""
    v, f = _mesh_operands(what, verts, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0 or V == 0:
        raise ValueError(f'{what}: a mesh of {F} faces and {V} vertices has no closest point')
    if grid is None:
        grid = mesh_face_grid(v, f)
    elif not isinstance(grid, FaceGrid) or not grid.matches(v, f):
        raise ValueError(f'{what}: grid must be the mesh_face_grid of these verts and faces')
    for name, t, dtype, shape in (('twin', twin, _I32, (3 * F,)), ('pseudonormals', pseudonormals, torch.float64, (V, 3))):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f'{what}: {name} must be a {dtype} tensor of shape {shape}, got '
                             f'{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}')
        if t.device != v.device or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous and on {v.device}')
    twin = mesh_edge_table(f, V).twin if twin is None else twin.detach()
    P = mesh_vertex_pseudonormals(v, f) if pseudonormals is None else pseudonormals.detach()
    return v, f, grid, twin, P


def _signed_distance(p, lattice, N, v, f, grid, twin, P, B, want_point, want_feature, want_stats=False):
    import ctypes
    V, F = int(v.shape[0]), int(f.shape[0])
    dev = v.device
    sdist = torch.empty(N, device=dev, dtype=_F32)
    face = torch.empty(N, device=dev, dtype=_I32)
    point = torch.empty((N, 3), device=dev, dtype=_F32) if want_point else None
    feature = torch.empty(N, device=dev, dtype=_I32) if want_feature else None
    stats = torch.empty(2, device=dev, dtype=torch.int64) if want_stats else None
    none = ptr(None)
    cbox = (ctypes.c_float * 6)(*[float(x) for x in grid.box])
    ccells = (ctypes.c_int * 3)(*grid.cells)
    if lattice is None:
        clo = ch = ccounts = None
    else:
        clo, ch = (ctypes.c_float * 3)(*[float(x) for x in lattice[0]]), (ctypes.c_float * 3)(*[float(x) for x in lattice[1]])
        ccounts = (ctypes.c_int * 3)(*lattice[2])
    call('mvip_mesh_signed_distance', ptr(p) if p is not None and N else none, clo, ch, ccounts, N, ptr(v), ptr(f, _I32), V, F, cbox,
         ccells, ptr(grid.cell_offsets, _I32), ptr(grid.cell_faces, _I32) if grid.n_pairs else none, grid.n_pairs, ptr(twin, _I32),
         ptr(P, torch.float64), B, ptr(sdist) if N else none, ptr(face, _I32) if N else none,
         ptr(point) if want_point and N else none, ptr(feature, _I32) if want_feature and N else none,
         ptr(stats, torch.int64) if want_stats else none, stream())
    return sdist, face, point, feature, stats


def mesh_signed_distance(points, verts, faces, grid=None, twin=None, pseudonormals=None, max_dist=None, return_feature=False,
                         return_stats=False):
    """The signed distance of each of points [N, 3] fp32 to the mesh (verts [V, 3] fp32, faces [F, 3] int32), all on the GPU:
    (sdist [N] fp32, face [N] int32, point [N, 3] fp32), with return_feature=True also feature [N] int32.  face, point and
    |sdist| are mesh_closest_point's; the sign is that of n . (p - q) with n the angle-weighted pseudonormal of the closest
    feature (csrc/mesh_sdf.hip, tests/mesh_sdf_numpy.py): the face normal, the sum of the two unit normals at an edge (feature
    1..3), the angle-weighted sum at a vertex (4..6).  Negative inside a closed mesh whose faces are counter-clockwise seen from
    outside; defined, by the same rule, on any mesh (mesh.topology says what the mesh is).  max_dist: queries farther than it
    get face -1 and NaN, as queries with a NaN or infinite coordinate do; the rest are unchanged by it.  grid / twin /
    pseudonormals: those of mesh_face_grid / mesh_edge_table / mesh_vertex_pseudonormals for these tensors (None: built here).
    A twin or pseudonormals that is given is checked for dtype, shape and device only and otherwise TRUSTED to be of this mesh:
    one of another mesh gives wrong signs (never an access out of range: the kernel bounds every index it reads from them).
    return_stats=True appends mesh_closest_point's [2] int64 counters (a counting variant of the kernel).
    ValueError as mesh_closest_point, and for max_dist < 0 or NaN.  Detached."""
    what = 'mesh_signed_distance'
    if not torch.is_tensor(points):
        raise ValueError(f'{what}: points must be a tensor on the GPU, got {type(points).__name__}')
    if points.dtype != _F32:
        raise ValueError(f'{what}: points must be {_F32}, got {points.dtype}')
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'{what}: points must be [N, 3], got {tuple(points.shape)}')
    p = points.detach()
    if not p.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if not p.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    N = int(p.shape[0])
    if 3 * N > 2 ** 31 - 1:
        raise ValueError(f'{what}: {N} points exceed int32 indices')
    B = _band(what, max_dist)
    if torch.is_tensor(verts) and p.device != verts.device:
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(verts.device), str(p.device)})}')
    v, f, grid, twin, P = _sdf_mesh(what, verts, faces, grid, twin, pseudonormals)
    sdist, face, point, feature, stats = _signed_distance(p, None, N, v, f, grid, twin, P, B, True, return_feature, return_stats)
    out = (sdist, face, point, feature) if return_feature else (sdist, face, point)
    return out + (stats,) if return_stats else out


def mesh_lattice(bound_min, bound_max, resolution):
    """(lo fp32 [3], h fp32 [3], counts (nx, ny, nz)) of the lattice of mesh.grid_axes: point i of an axis is fp32(fp32(i) h) + lo,
    h = (hi - lo) / fp32(n - 1) in fp32.  Host code.  ValueError for a count below 2, non-finite bounds, a step that is not > 0,
    more than 2^31 - 1 points."""
    import numpy as np
    what = 'mesh_signed_distance_lattice'
    lo, hi = np.asarray(bound_min, np.float32).reshape(-1), np.asarray(bound_max, np.float32).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError(f'{what}: bound_min / bound_max must be three finite numbers each')
    counts = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)
    if len(counts) != 3 or min(counts) < 2:
        raise ValueError(f'{what}: resolution must be one or three counts >= 2, got {resolution!r}')
    if counts[0] * counts[1] * counts[2] > 2 ** 31 - 1:
        raise ValueError(f'{what}: {counts} lattice points exceed int32 indices')
    with np.errstate(over='ignore', invalid='ignore'):
        h = np.asarray([(hi[a] - lo[a]) / np.float32(counts[a] - 1) for a in range(3)], np.float32)
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        raise ValueError(f'{what}: the box {lo.tolist()} .. {hi.tolist()} has no finite step > 0 on {counts} points')
    return lo, h, counts


def mesh_signed_distance_lattice(verts, faces, bound_min, bound_max, resolution, max_dist=None, grid=None, twin=None,
                                 pseudonormals=None, return_stats=False):
    """mesh_signed_distance on the lattice of mesh.grid_axes(bound_min, bound_max, resolution) without the [N, 3] tensor of its
    points (the kernel generates them, bit for bit those of grid_axes): (sdist [nx, ny, nz] fp32, face [nx, ny, nz] int32).
    With max_dist the walk of a far point ends as soon as nothing within max_dist can remain: a narrow band of a large lattice
    costs little more than its in-band points.  return_stats=True appends the [2] int64 counters.  ValueError as mesh_signed_distance and mesh_lattice."""
    what = 'mesh_signed_distance_lattice'
    lattice = mesh_lattice(bound_min, bound_max, resolution)
    B = _band(what, max_dist)
    v, f, grid, twin, P = _sdf_mesh(what, verts, faces, grid, twin, pseudonormals)
    counts = lattice[2]
    sdist, face, _, _, stats = _signed_distance(None, lattice, counts[0] * counts[1] * counts[2], v, f, grid, twin, P, B, False, False,
                                                return_stats)
    return (sdist.view(counts), face.view(counts), stats) if return_stats else (sdist.view(counts), face.view(counts))


# mesh ray casting: first hit, occlusion, face openness on the face grid (beyond the reference, csrc/mesh_raycast.hip) ---------------
# The definition is csrc/mesh_raycast.hip's and tests/mesh_raycast_numpy.py's.  There is no CPU path.

MESH_OPENNESS_MAX_DIRECTIONS = 255


def _ray_operand(what, name, t, width, dev, dtype=None):
    dtype = _F32 if dtype is None else dtype
    if not torch.is_tensor(t):
        raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
    if t.dtype != dtype:
        raise ValueError(f'{what}: {name} must be {dtype}, got {t.dtype}')
    if (t.dim() != 2 or t.shape[1] != width) if width else t.dim() != 1:
        raise ValueError(f'{what}: {name} must be {"[N, %d]" % width if width else "[N]"}, got {tuple(t.shape)}')
    t = t.detach()
    if not t.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if t.device != dev:
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(dev), str(t.device)})}')
    if not t.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    return t


def _ray_grid(what, v, f, grid):
    """the FaceGrid of (v, f) with its vertex bounds, and the host arrays of the C ABI"""
    import ctypes
    import numpy as np
    if grid is None:
        grid = mesh_face_grid(v, f)
    elif not isinstance(grid, FaceGrid) or not grid.matches(v, f):
        raise ValueError(f'{what}: grid must be the mesh_face_grid of these verts and faces')
    if grid.bounds is None:
        grid.bounds = torch.stack([v.amin(0), v.amax(0)]).cpu().numpy().reshape(6).astype(np.float32)
    cbox = (ctypes.c_float * 6)(*[float(x) for x in grid.box])
    ccells = (ctypes.c_int * 3)(*grid.cells)
    cbounds = (ctypes.c_float * 6)(*[float(x) for x in grid.bounds])
    return grid, cbox, ccells, cbounds


def _cast(what, any_hit, origins, dirs, verts, faces, tmin, tmax, skip, grid, return_bary, return_stats):
    import math
    v, f = _mesh_operands(what, verts, faces)
    dev = v.device
    o = _ray_operand(what, 'origins', origins, 3, dev)
    d = _ray_operand(what, 'dirs', dirs, 3, dev)
    N = int(o.shape[0])
    if d.shape[0] != N:
        raise ValueError(f'{what}: {N} origins but {int(d.shape[0])} dirs')
    if 3 * N > 2 ** 31 - 1:
        raise ValueError(f'{what}: {N} rays exceed int32 indices')
    lims = []
    for name, lim in (('tmin', tmin), ('tmax', tmax)):
        if torch.is_tensor(lim):
            lim = _ray_operand(what, name, lim, 0, dev)
            if lim.shape[0] != N:
                raise ValueError(f'{what}: {name} must be a number or [{N}], got {tuple(lim.shape)}')
            lims.append((lim, 0.0))
        else:
            if isinstance(lim, bool) or not isinstance(lim, (int, float)) or math.isnan(float(lim)):
                raise ValueError(f'{what}: {name} must be a number or a [N] tensor, got {lim!r}')
            lims.append((None, float(lim)))
    if skip is not None:
        skip = _ray_operand(what, 'skip', skip, 0, dev, _I32)
        if skip.shape[0] != N:
            raise ValueError(f'{what}: skip must be [{N}], got {tuple(skip.shape)}')
    if int(f.shape[0]) == 0 or int(v.shape[0]) == 0:
        raise ValueError(f'{what}: a mesh of {int(f.shape[0])} faces and {int(v.shape[0])} vertices cannot be hit')
    grid, cbox, ccells, cbounds = _ray_grid(what, v, f, grid)
    V, F = int(v.shape[0]), int(f.shape[0])
    face = torch.empty(N, device=dev, dtype=_I32)
    t = None if any_hit else torch.empty(N, device=dev, dtype=_F32)
    bary = torch.empty((N, 2), device=dev, dtype=_F32) if return_bary else None
    stats = torch.empty(3, device=dev, dtype=torch.int64) if return_stats else None
    none = ptr(None)
    some = lambda x, dt=_F32: ptr(x, dt) if (x is not None and N) else none
    call('mvip_mesh_raycast', some(o), some(d), some(lims[0][0]), some(lims[1][0]), lims[0][1], lims[1][1], some(skip, _I32), N,
         ptr(v), ptr(f, _I32), V, F, cbox, ccells, cbounds, ptr(grid.cell_offsets, _I32),
         ptr(grid.cell_faces, _I32) if grid.n_pairs else none, grid.n_pairs, 1 if any_hit else 0, some(face, _I32), some(t),
         some(bary), ptr(stats, torch.int64) if return_stats else none, stream())
    return face, t, bary, stats


def mesh_cast_rays(origins, dirs, verts, faces, tmin=0., tmax=float('inf'), skip=None, grid=None, return_bary=False,
                   return_stats=False):
    """The first face of the mesh (verts [V, 3] fp32, faces [F, 3] int32) that each ray hits: (face [N] int32, t [N] fp32), all on
    the GPU.  origins / dirs [N, 3] fp32; tmin / tmax numbers or [N] fp32 tensors; skip [N] int32 or None: one face per ray that
    never counts (-1: none).  The definition (csrc/mesh_raycast.hip, tests/mesh_raycast_numpy.py): the watertight ray-triangle
    test in fp64 on the widened inputs, no culling; the hit of smallest t in [tmin, tmax], the lowest face index among equals;
    face -1 and t +inf for a miss; face -1 and t NaN for an invalid ray (a NaN or infinite origin or direction, a zero
    direction, tmin not finite, tmax NaN or < tmin).  return_bary=True appends bary [N, 2] fp32, the weights of the face's
    second and third vertex (NaN without a hit).  grid: a FaceGrid of mesh_face_grid for these very tensors (None: built
    here); the result does not depend on it.  return_stats=True appends a [3] int64 device tensor (a counting variant of the
    kernel): the ray-face tests, 64 times the tests of each wave's busiest lane summed over the waves, the cells visited.
    N = 0 gives empty tensors.  ValueError for bad shapes or dtypes, CPU tensors, F = 0, a face index outside [0, V), a NaN or
    infinite vertex, a grid of another mesh.  Detached."""
    face, t, bary, stats = _cast('mesh_cast_rays', False, origins, dirs, verts, faces, tmin, tmax, skip, grid, return_bary,
                                 return_stats)
    return (face, t) + ((bary,) if return_bary else ()) + ((stats,) if return_stats else ())


def mesh_occluded(origins, dirs, verts, faces, tmin=0., tmax=float('inf'), skip=None, grid=None, return_stats=False):
    """[N] bool: does the ray hit any face -- face >= 0 of mesh_cast_rays, by a kernel that stops at the first accepted hit.  An
    invalid ray is not occluded.  Arguments and errors as mesh_cast_rays; return_stats=True returns (occluded, stats)."""
    face, _, _, stats = _cast('mesh_occluded', True, origins, dirs, verts, faces, tmin, tmax, skip, grid, False, return_stats)
    return (face >= 0, stats) if return_stats else face >= 0


def mesh_face_openness(verts, faces, directions, max_dist=float('inf'), grid=None, return_stats=False):
    """Per face, in how many of the directions [K, 3] fp32 (K <= 255, finite, on the GPU) it sees nothing: (front_open,
    front_total, back_open, back_total), each int32 [F].  The definition (csrc/mesh_raycast.hip): the ray from the fp64
    centroid ((a + b) + c) / 3 along d_k over [0, max_dist] with the face itself skipped; d_k counts for the front side iff
    N . d_k > 0, N = (b - a) x (c - a), for the back side iff < 0, for neither iff == 0; open iff the ray hits nothing.  The rays
    are generated in the kernel, one thread per face.  F = 0 gives empty tensors.  return_stats as mesh_cast_rays.  ValueError
    for bad shapes or dtypes, K > 255, a NaN or infinite direction, max_dist NaN or < 0, a grid of another mesh."""
    import math
    what = 'mesh_face_openness'
    v, f = _mesh_operands(what, verts, faces)
    dev = v.device
    d = _ray_operand(what, 'directions', directions, 3, dev)
    K = int(d.shape[0])
    if K > MESH_OPENNESS_MAX_DIRECTIONS:
        raise ValueError(f'{what}: at most {MESH_OPENNESS_MAX_DIRECTIONS} directions, got {K}')
    if K and not bool(torch.isfinite(d).all()):
        raise ValueError(f'{what}: a direction is NaN or infinite')
    if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float)) or math.isnan(float(max_dist)) or max_dist < 0:
        raise ValueError(f'{what}: max_dist must be a number >= 0 (inf: no limit), got {max_dist!r}')
    V, F = int(v.shape[0]), int(f.shape[0])
    if F == 0:
        if grid is not None:
            raise ValueError(f'{what}: grid must be the mesh_face_grid of these verts and faces')
        z = torch.zeros(0, device=dev, dtype=_I32)
        return (z, z.clone(), z.clone(), z.clone()) + ((torch.zeros(3, device=dev, dtype=torch.int64),) if return_stats else ())
    if 4 * F > 2 ** 31 - 1:
        raise ValueError(f'{what}: {F} faces exceed int32 indices')
    grid, cbox, ccells, cbounds = _ray_grid(what, v, f, grid)
    counts = torch.empty((4, F), device=dev, dtype=_I32)
    stats = torch.empty(3, device=dev, dtype=torch.int64) if return_stats else None
    none = ptr(None)
    call('mvip_mesh_face_openness', ptr(v), ptr(f, _I32), V, F, cbox, ccells, cbounds, ptr(grid.cell_offsets, _I32),
         ptr(grid.cell_faces, _I32) if grid.n_pairs else none, grid.n_pairs, ptr(d) if K else none, K, float(max_dist),
         ptr(counts, _I32), ptr(stats, torch.int64) if return_stats else none, stream())
    out = (counts[0], counts[1], counts[2], counts[3])
    return out + ((stats,) if return_stats else ())


# mesh rasterisation: disparity, face ids and colours per view (beyond the reference, csrc/raster.hip) -------------------------------
# The definition is csrc/raster.hip's and tests/raster_numpy.py's.  There is no CPU path.

RASTER_CULLS = ('none', 'back')
RASTER_MAX_SIDE = 16384


def mesh_rasterize(verts, faces, poses, H, W, focal, near=1e-3, cull='none', colors=None, stats=False):
    """Rasterise an indexed mesh into V cameras: (disp [V, H, W] fp32, face [V, H, W] int32, rgb [V, H, W, 3] uint8 or None).
    verts [Nv, 3] fp32, faces [F, 3] int32 (counter-clockwise seen from outside), poses [V, 3, 4] fp32 camera-to-world, colors
    [Nv, 3] uint8 or None, all on the GPU; the camera conventions are tsdf_fuse's (looking down -z, no half-pixel offset).  disp
    is 1 / planar depth of the nearest face at the pixel centre and 0 where nothing covers it, face the index of that face and
    -1, rgb the perspective-correct interpolation of its vertex colours and 0.  8 sub-pixel bits and the top-left fill rule: two
    faces that share an edge never both cover a pixel and never both miss it; equal disparities go to the lower face index,
    so the result does not depend on the order of the atomics and a call equals its repetition bit for bit.  cull='back' drops
    the faces seen from inside.  THERE IS NO NEAR-PLANE CLIPPING: a face with a vertex nearer than `near` (or behind the
    camera, or more than 16,384 pixels off the image centre's axes) is dropped whole for that view.  H, W in 1..16384; focal
    and near finite and > 0.  V = 0, F = 0 and Nv = 0 give empty maps.  ValueError for bad shapes or dtypes, CPU tensors, or a
    face index outside [0, Nv) (checked on the device, one flag read back: the only synchronisation).  stats=True appends
    (fragments, atomics sent) as a [2] int64 device tensor, from a counting variant of the fragment kernel.  Two launches and
    one clear.  Detached."""
    import math
    what = 'mesh_rasterize'
    v, f, *rest = _mesh_operands(what, verts, faces, colors)
    c = rest[0] if rest else None
    p = _pose_batch(what, poses, 'poses')
    if not p.is_cuda:
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if p.device != v.device:
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(v.device), str(p.device)})}')
    if not p.is_contiguous():
        raise ValueError(f'{what}: every operand must be contiguous')
    if int(H) != H or int(W) != W or not (1 <= int(H) <= RASTER_MAX_SIDE and 1 <= int(W) <= RASTER_MAX_SIDE):
        raise ValueError(f'{what}: H and W must be integers in 1..{RASTER_MAX_SIDE}, got {H!r} x {W!r}')
    H, W, focal, near = int(H), int(W), float(focal), float(near)
    if not (math.isfinite(focal) and focal > 0 and math.isfinite(near) and near > 0):
        raise ValueError(f'{what}: focal {focal} and near {near} must be finite and > 0')
    if cull not in RASTER_CULLS:
        raise ValueError(f'{what}: cull must be one of {RASTER_CULLS}, got {cull!r}')
    Nv, F, V = int(v.shape[0]), int(f.shape[0]), int(p.shape[0])
    dev = v.device
    disp = torch.empty((V, H, W), device=dev, dtype=_F32)
    face = torch.empty((V, H, W), device=dev, dtype=_I32)
    rgb = torch.empty((V, H, W, 3), device=dev, dtype=torch.uint8) if c is not None else None
    keys = torch.empty((V, H, W), device=dev, dtype=torch.int64)
    flag = torch.empty(1, device=dev, dtype=_I32)
    counts = torch.empty(2, device=dev, dtype=torch.int64) if stats else None
    none = ptr(None)
    args = (ptr(v) if Nv else none, ptr(f, _I32) if F else none)
    geom = (Nv, F, ptr(p) if V else none, V, H, W, focal, near)
    call('mvip_raster_fragments', *args, *geom, RASTER_CULLS.index(cull), ptr(keys, torch.int64) if V else none, ptr(flag, _I32),
         ptr(counts, torch.int64) if stats else none, stream())
    call('mvip_raster_resolve', ptr(keys, torch.int64) if V else none, *args, ptr(c, torch.uint8) if c is not None and Nv else none,
         *geom, ptr(disp) if V else none, ptr(face, _I32) if V else none, ptr(rgb, torch.uint8) if c is not None and V else none,
         stream())
    if int(flag.cpu()):
        raise ValueError(f'{what}: a face index lies outside [0, {Nv})')
    return (disp, face, rgb, counts) if stats else (disp, face, rgb)


# mesh texturing: colours baked from the views, a per-face atlas, the textured render (beyond the reference, csrc/texture.hip) ---------
# The definition is csrc/texture.hip's and tests/texture_numpy.py's.  There is no CPU path.

TEXTURE_MODES = ('blend', 'best')
TEXTURE_ORDERS = ('row', 'block')
TEXTURE_MAX_TEXELS = 32


def texture_layout(n_faces, texels):
    """(Ht, Wt, Bx, By, S) of the atlas of n_faces faces at `texels` texels along a leg: the layout of csrc/texture.hip, in
    integers.  ValueError for texels outside 1..32 or a texture side over 16,384."""
    F = int(n_faces)
    if int(texels) != texels or not 1 <= int(texels) <= TEXTURE_MAX_TEXELS or F < 0:
        raise ValueError(f'texture_layout: texels must be an integer in 1..{TEXTURE_MAX_TEXELS} and F >= 0, got {texels!r}, {F}')
    S = int(texels) + 3
    B = (F + 1) // 2
    Bx = 0
    while Bx * Bx < B:
        Bx += 1
    By = -(-B // Bx) if Bx else 0
    if Bx * S > RASTER_MAX_SIDE or By * S > RASTER_MAX_SIDE:
        raise ValueError(f'texture_layout: {F} faces at {texels} texels need a texture of {By * S} x {Bx * S}: a side over {RASTER_MAX_SIDE}')
    return By * S, Bx * S, Bx, By, S


def _bake_views(what, dev, images, disp, poses, focal, near, tol, cull, mode, masks):
    """The checks the two bakes share: (images, disp, poses, masks or None, V, H, W, focal, near, tol, cull index, mode index)."""
    import math
    d = _image_batch(what, disp, _F32, 'disp')
    p = _pose_batch(what, poses, 'poses')
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        got = f'{tuple(images.shape)} {images.dtype}' if torch.is_tensor(images) else type(images).__name__
        raise ValueError(f'{what}: images must be a torch.uint8 tensor [V, H, W, 3] on the GPU, got {got}')
    im = images.detach()
    tensors = [im, d, p]
    if masks is not None:
        tensors.append(_image_batch(what, masks, torch.bool, 'masks'))
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if any(t.device != dev for t in tensors):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(dev)} | {str(t.device) for t in tensors})}')
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: every operand must be contiguous')
    V, H, W = (int(x) for x in d.shape)
    if tuple(im.shape) != (V, H, W, 3) or p.shape[0] != V or (masks is not None and tuple(tensors[3].shape) != (V, H, W)):
        raise ValueError(f'{what}: images {tuple(im.shape)}, disp {tuple(d.shape)}, poses {tuple(p.shape)}'
                         + (f', masks {tuple(tensors[3].shape)}' if masks is not None else '') + ': one V, H, W expected')
    if not (1 <= H <= RASTER_MAX_SIDE and 1 <= W <= RASTER_MAX_SIDE):
        raise ValueError(f'{what}: H and W must be in 1..{RASTER_MAX_SIDE}, got {H} x {W}')
    focal, near, tol = float(focal), float(near), float(tol)
    if not (math.isfinite(focal) and focal > 0 and math.isfinite(near) and near > 0):
        raise ValueError(f'{what}: focal {focal} and near {near} must be finite and > 0')
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f'{what}: tol {tol} must be finite and >= 0')
    if cull not in RASTER_CULLS:
        raise ValueError(f'{what}: cull must be one of {RASTER_CULLS}, got {cull!r}')
    if mode not in TEXTURE_MODES:
        raise ValueError(f'{what}: mode must be one of {TEXTURE_MODES}, got {mode!r}')
    return im, d, p, (tensors[3] if masks is not None else None), V, H, W, focal, near, tol, RASTER_CULLS.index(cull), TEXTURE_MODES.index(mode)


def _view_args(im, d, m, p, V, H, W, focal, near, tol, cull, mode):
    none = ptr(None)
    return (ptr(im, torch.uint8) if V else none, ptr(d) if V else none, ptr(m, torch.bool) if m is not None and V else none,
            ptr(p) if V else none, V, H, W, focal, near, tol, cull, mode)


def mesh_bake_points(points, normals, images, disp, poses, focal, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None):
    """Colours for N sample points of a mesh from V views: (rgb [N, 3] uint8, wsum [N] fp32, best [N] int32).  points, normals
    [N, 3] fp32 (the normals need no unit length), images [V, H, W, 3] uint8, disp [V, H, W] fp32: the disparities of the SAME
    mesh rasterised into poses [V, 3, 4] (mesh_rasterize), masks [V, H, W] bool or None (False = ignore the pixel), all on the
    GPU.  A view contributes to a point iff the point projects inside the image at planar depth >= near, faces the camera
    (cull='back': nrm . (o - p) > 0; 'none': != 0) and at all four pixels of its bilinear footprint the disparity D is that of
    the point's own surface, |D z - 1| <= tol (warp_views' test and default) and the mask True: a footprint that straddles an
    occlusion edge takes nothing from that view.  The colour is the bilinear value of the image, the weight cos^2 of the
    incidence.  mode='blend': the weighted mean over the views, 'best': the colour of the view of largest weight (the lower
    index on a tie).  wsum = the sum of the weights (0: no view sees the point, rgb is 0), best = the view of largest weight or
    -1.  fp64 throughout: a call equals its repetition and tests/texture_numpy.py bit for bit.  ValueError for bad shapes,
    dtypes, CPU tensors or mixed devices.  One launch.  Detached."""
    what = 'mesh_bake_points'
    named = (('points', points), ('normals', normals))
    for name, t in named:
        if not torch.is_tensor(t):
            raise ValueError(f'{what}: {name} must be a tensor on the GPU, got {type(t).__name__}')
        if t.dtype != _F32:
            raise ValueError(f'{what}: {name} must be {_F32}, got {t.dtype}')
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f'{what}: {name} must be [N, 3], got {tuple(t.shape)}')
    pt, nr = points.detach(), normals.detach()
    if not (pt.is_cuda and nr.is_cuda):
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if pt.shape != nr.shape or pt.device != nr.device:
        raise ValueError(f'{what}: points {tuple(pt.shape)} on {pt.device} and normals {tuple(nr.shape)} on {nr.device}: one shape on one device expected')
    if not (pt.is_contiguous() and nr.is_contiguous()):
        raise ValueError(f'{what}: every operand must be contiguous')
    im, d, p, m, *geom = _bake_views(what, pt.device, images, disp, poses, focal, near, tol, cull, mode, masks)
    n = int(pt.shape[0])
    dev = pt.device
    rgb = torch.empty((n, 3), device=dev, dtype=torch.uint8)
    wsum = torch.empty(n, device=dev, dtype=_F32)
    best = torch.empty(n, device=dev, dtype=_I32)
    none = ptr(None)
    call('mvip_texture_bake_points', ptr(pt) if n else none, ptr(nr) if n else none, n, *_view_args(im, d, m, p, *geom),
         ptr(rgb, torch.uint8) if n else none, ptr(wsum) if n else none, ptr(best, _I32) if n else none, stream())
    return rgb, wsum, best


def mesh_bake_atlas(verts, faces, texels, images, disp, poses, focal, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None,
                    order='block'):
    """The texture atlas of a mesh baked from V views: (rgb [Ht, Wt, 3] uint8, wsum [Ht, Wt] fp32, best [Ht, Wt] int32), (Ht, Wt) =
    texture_layout(F, texels)[:2].  Faces 2k and 2k + 1 share a block of (texels + 3)^2 texels; every owned texel is the bake
    of mesh_bake_points at a point of its face (the barycentric lattice of `texels` steps along a leg; gutter texels take the
    nearest point of the closed face) with the face's own fp64 normal (p1 - p0) x (p2 - p0), derived from the texel index:
    nothing is materialised.  Texels without an owner hold 0 / 0 / -1.  verts [Nv, 3] fp32, faces [F, 3] int32; the views as in
    mesh_bake_points.  order: how texels map to lanes ('block', the default: the texels of a block are consecutive, 11 to 19 % faster than 'row',
    texture row-major, in tools/mesh_texture_bench.py), the same output.
    ValueError for bad shapes, dtypes, CPU tensors, mixed devices, or a face index outside [0, Nv) (one flag read back: the only
    synchronisation).  One launch and the flag's clear.  Detached."""
    what = 'mesh_bake_atlas'
    v, f = _mesh_operands(what, verts, faces)
    im, d, p, m, *geom = _bake_views(what, v.device, images, disp, poses, focal, near, tol, cull, mode, masks)
    if order not in TEXTURE_ORDERS:
        raise ValueError(f'{what}: order must be one of {TEXTURE_ORDERS}, got {order!r}')
    Nv, F = int(v.shape[0]), int(f.shape[0])
    Ht, Wt = texture_layout(F, texels)[:2]
    dev = v.device
    rgb = torch.empty((Ht, Wt, 3), device=dev, dtype=torch.uint8)
    wsum = torch.empty((Ht, Wt), device=dev, dtype=_F32)
    best = torch.empty((Ht, Wt), device=dev, dtype=_I32)
    flag = torch.empty(1, device=dev, dtype=_I32)
    none = ptr(None)
    call('mvip_texture_bake_atlas', ptr(v) if Nv else none, ptr(f, _I32) if F else none, Nv, F, int(texels), TEXTURE_ORDERS.index(order),
         *_view_args(im, d, m, p, *geom), ptr(rgb, torch.uint8) if F else none, ptr(wsum) if F else none,
         ptr(best, _I32) if F else none, ptr(flag, _I32), stream())
    if int(flag.cpu()):
        raise ValueError(f'{what}: a face index lies outside [0, {Nv})')
    return rgb, wsum, best


def mesh_texture_resolve(face, verts, faces, atlas, texels, poses, focal, near=1e-3):
    """rgb [V, H, W, 3] uint8 of a textured mesh for the face maps face [V, H, W] int32 that mesh_rasterize gave for the same verts
    [Nv, 3], faces [F, 3], poses [V, 3, 4], focal and near: per covered pixel the winner's perspective-correct barycentrics are
    recomputed as the rasteriser's colour resolve does, mapped to the face's half block of atlas [Ht, Wt, 3] uint8 (the layout of
    mesh_bake_atlas at `texels`) and the atlas is read bilinearly.  0 where face < 0 (or not a face of the mesh).  ValueError for
    bad shapes, dtypes, CPU tensors or mixed devices.  One launch.  Detached."""
    import math
    what = 'mesh_texture_resolve'
    v, f = _mesh_operands(what, verts, faces)
    fm = _image_batch(what, face, _I32, 'face')
    p = _pose_batch(what, poses, 'poses')
    Nv, F = int(v.shape[0]), int(f.shape[0])
    Ht, Wt = texture_layout(F, texels)[:2]
    if not torch.is_tensor(atlas) or atlas.dtype != torch.uint8 or tuple(atlas.shape) != (Ht, Wt, 3):
        got = f'{tuple(atlas.shape)} {atlas.dtype}' if torch.is_tensor(atlas) else type(atlas).__name__
        raise ValueError(f'{what}: atlas must be a torch.uint8 tensor [{Ht}, {Wt}, 3] on the GPU, got {got}')
    a = atlas.detach()
    if not all(t.is_cuda for t in (fm, p, a)):
        raise ValueError(f'{what}: tensors on the GPU expected (the HIP path has no CPU path)')
    if any(t.device != v.device for t in (fm, p, a)):
        raise ValueError(f'{what}: tensors on one device expected, got {sorted({str(t.device) for t in (v, fm, p, a)})}')
    if not all(t.is_contiguous() for t in (fm, p, a)):
        raise ValueError(f'{what}: every operand must be contiguous')
    V, H, W = (int(x) for x in fm.shape)
    if p.shape[0] != V:
        raise ValueError(f'{what}: face {tuple(fm.shape)} and poses {tuple(p.shape)}: one V expected')
    if not (1 <= H <= RASTER_MAX_SIDE and 1 <= W <= RASTER_MAX_SIDE):
        raise ValueError(f'{what}: H and W must be in 1..{RASTER_MAX_SIDE}, got {H} x {W}')
    focal, near = float(focal), float(near)
    if not (math.isfinite(focal) and focal > 0 and math.isfinite(near) and near > 0):
        raise ValueError(f'{what}: focal {focal} and near {near} must be finite and > 0')
    rgb = torch.empty((V, H, W, 3), device=v.device, dtype=torch.uint8)
    none = ptr(None)
    call('mvip_texture_resolve', ptr(fm, _I32) if V else none, ptr(v) if Nv else none, ptr(f, _I32) if F else none, Nv, F,
         ptr(a, torch.uint8) if F else none, int(texels), ptr(p) if V else none, V, H, W, focal, near,
         ptr(rgb, torch.uint8) if V else none, stream())
    return rgb


# mesh voxelisation: the cells a mesh's faces touch and the cells inside it, as bit-grid words (beyond the reference,
# csrc/mesh_voxel.hip) ---------------------------------------------------------------------------------------------------------
# The definitions are csrc/mesh_voxel.hip's and tests/voxel_numpy.py's.  There is no CPU path.

VOXEL_AXES = ('x', 'y', 'z', 'majority')
VOXEL_COUNTERS = 5                 # flag, dropped, odd columns x / y / z (csrc/mesh_voxel.hip: N_COUNTERS)


def _voxel_args(what, verts, faces, box, cells):
    import ctypes
    import math
    import numpy as np
    v, f = _mesh_operands(what, verts, faces)
    try:
        box = [float(b) for b in box]
        cells = [int(c) for c in cells]
    except (TypeError, ValueError):
        raise ValueError(f'{what}: box must be six numbers (bmin, inv) and cells three integers') from None
    if len(box) != 6 or len(cells) != 3 or not all(1 <= c <= 512 for c in cells):
        raise ValueError(f'{what}: box must be six numbers (bmin, inv) and cells three integers in 1..512, got {box} and {cells}')
    with np.errstate(over='ignore'):
        box32 = [float(np.float32(b)) for b in box]
    if not all(math.isfinite(b) for b in box32) or not all(b > 0 for b in box32[3:]):
        raise ValueError(f'{what}: box {box}: bmin must be finite and inv finite and > 0 in fp32')
    return v, f, (ctypes.c_float * 6)(*box32), (ctypes.c_int * 3)(*cells), tuple(cells)


def mesh_voxelize_surface(verts, faces, box, cells):
    """(words, dropped): the cells of a bit grid that the faces of an indexed mesh touch, conservatively.  verts [Nv, 3] fp32 and
    faces [F, 3] int32 on the GPU; box = (bmin[3], inv[3]) as BitGrid.box() gives it and cells three integers in 1..512 (host).
    words: int32 [(cx cy cz + 31) // 32] in the layout of bitgrid.py.  A cell is set iff some face overlaps the cell grown by
    2^-12 of a cell on every side (the exact triangle-box test in fp64, csrc/mesh_voxel.hip), so every fp32 point of a face that
    the renderer's own cell lookup places in the box lies in a set cell.  dropped: the number of faces with a non-finite vertex
    (they mark nothing).  F = 0 and Nv = 0 give a clear grid.  ValueError for bad shapes or dtypes, CPU tensors, a bad box or
    cells, or a face index outside [0, Nv) (checked on the device; the counters are read back once: the only synchronisation).
    Integer OR marks: a call equals its repetition bit for bit.  Detached."""
    what = 'mesh_voxelize_surface'
    v, f, cbox, ccells, cells = _voxel_args(what, verts, faces, box, cells)
    Nv, F = int(v.shape[0]), int(f.shape[0])
    words = torch.empty(occupancy_words(cells), device=v.device, dtype=_I32)
    counters = torch.empty(VOXEL_COUNTERS, device=v.device, dtype=_I32)
    none = ptr(None)
    call('mvip_voxel_surface', ptr(v) if Nv else none, ptr(f, _I32) if F else none, Nv, F, cbox, ccells, ptr(words, _I32),
         ptr(counters, _I32), stream())
    c = counters.cpu().tolist()
    if c[0]:
        raise ValueError(f'{what}: a face index lies outside [0, {Nv})')
    return words, c[1]


def mesh_voxelize_solid(verts, faces, box, cells, axes='majority'):
    """(words, odd_columns, dropped): the cells of a bit grid whose centres lie inside an indexed mesh, by the parity of the
    crossings of the cell columns along `axes`: 'x', 'y' or 'z' alone, or 'majority' -- all three, a cell set iff at least two
    agree (operands as mesh_voxelize_surface).  Vertices are snapped to 8 sub-cell bits and coverage is decided in integers with
    the rasteriser's ownership rule (csrc/mesh_voxel.hip): for a closed mesh every column is even and a centre farther than 2^-8
    of a cell from the surface gets the exact answer; a hole leaks whole column segments on a single axis, and under 'majority'
    changes nothing outside the missing faces' bounding boxes.  odd_columns: a list of three integers, the columns of odd total
    parity per axis (0 for an axis not walked) -- the leak diagnostic.  dropped: the faces left out whole because a vertex is
    not finite or lies more than 16,384 cells from the box origin on a rastered axis.  ValueError as mesh_voxelize_surface, and
    for an unknown `axes`.  Integer XOR marks: a call equals its repetition bit for bit.  Detached."""
    what = 'mesh_voxelize_solid'
    v, f, cbox, ccells, cells = _voxel_args(what, verts, faces, box, cells)
    if axes not in VOXEL_AXES:
        raise ValueError(f'{what}: axes must be one of {VOXEL_AXES}, got {axes!r}')
    a = VOXEL_AXES.index(axes)
    Nv, F = int(v.shape[0]), int(f.shape[0])
    n_scratch = _lib.load().mvip_voxel_scratch_words(ccells, a)
    if n_scratch < 0:
        raise _lib.MvipError(f'{what}: no scratch size for cells {cells}')
    scratch = torch.empty(n_scratch, device=v.device, dtype=_I32)
    words = torch.empty(occupancy_words(cells), device=v.device, dtype=_I32)
    counters = torch.empty(VOXEL_COUNTERS, device=v.device, dtype=_I32)
    none = ptr(None)
    call('mvip_voxel_crossings', ptr(v) if Nv else none, ptr(f, _I32) if F else none, Nv, F, cbox, ccells, a, ptr(scratch, _I32),
         ptr(counters, _I32), stream())
    call('mvip_voxel_fill', ptr(scratch, _I32), ccells, a, ptr(words, _I32), ptr(counters, _I32), stream())
    c = counters.cpu().tolist()
    if c[0]:
        raise ValueError(f'{what}: a face index lies outside [0, {Nv})')
    return words, c[2:5], c[1]
