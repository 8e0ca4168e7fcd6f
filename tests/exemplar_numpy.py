"""Exemplar-based (PatchMatch) image inpainting restated in numpy: the definition of csrc/exemplar.hip / ops.exemplar_fill,
vectorised over the targets.  Everything after the quantisation is integer arithmetic, so the HIP path must agree bit for bit.

Per image [H, W, 3] fp32 with mask [H, W], patch side P odd, r = P // 2:
  quantise  q = rint(clip(v, 0, 1) * 255) in fp32 (rint: ties to even, numpy's round); a pixel with a non-finite channel joins
            the hole; hole pixels start as 0.  `bad` = hole, or outside `sources` when that is given.
  sets      a centre is inside if its P x P patch lies in the image; T = inside centres whose patch holds a hole pixel,
            S = inside centres whose patch holds no bad pixel.  S empty at level 0: singular, returned unchanged.
  pyramid   level l + 1 is [h // 2, w // 2] (an odd last row / column is dropped): the colour is the round-half-up mean of the
            KNOWN pixels of the 2 x 2 block, (2 sum + n) // (2 n) (0 when none is known), hole = any of the four is hole,
            bad = any of the four is bad.  A level is added while min(h, w) // 2 >= 4 P, fewer than max_levels levels exist and
            the coarser level has a source.
  hash      lowbias32 chained: h = mix(seed ^ 0x9e3779b9); h = mix(h + level); h = mix(h + iteration); h = mix(h + k);
            h = mix(h + pixel) in uint32, pixel = y * w + x of the target at that level.  The initial pick uses
            iteration = 0xffffffff, k = 0.
  initial   coarsest level: s(t) = the (hash mod |S|)-th source in row-major order.  Finer level: the parent (ty >> 1, tx >> 1)
            when it is in the coarser image and was a target there gives 2 s_parent + (ty & 1, tx & 1), clamped to the inside
            centres; taken if it is in S, else the hashed pick.  Then one vote.
  search    Jacobi (reads the NNF of the previous iteration), candidates in the order: s(t); for st in 1, 2, 4 and (dy, dx) in
            (0, -st), (0, +st), (-st, 0), (+st, 0): s_old(t + d) - d if t + d is in T; random: s_best + (ry, rx) for R = max(h, w),
            R // 2, ... >= 1 (k = 0, 1, ...), ry = (hash & 0xffff) % (2R + 1) - R, rx = (hash >> 16) % (2R + 1) - R.  A candidate
            counts if it is in S, and replaces the best if its SSD (patch, three channels, integers) is strictly smaller.
            `iteration` counts the search iterations of the level from 0 across the rounds.
  vote      hole pixel p = (2 sum + n) // (2 n) over the n targets t = p - d, d in [-r, r]^2, that are in T, of img[s(t) + d].
  schedule  per level: initial, vote, then `rounds` x (`iters` searches, vote).
  output    known pixels bit for bit, hole pixels k / 255 in fp32; nnf [H, W, 2] = (sy, sx), -1 off T; energy = the sum over T of
            the SSD of (t, s(t)) on the final image.
"""
import numpy as np

M32 = np.uint64(0xffffffff)
INIT = 0xffffffff


def lowbias32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def hash5(seed, level, iteration, k, pixel):
    h = lowbias32(np.uint64((int(seed) & 0xffffffff) ^ 0x9e3779b9))
    h = lowbias32(h + np.uint64(level))
    h = lowbias32(h + np.uint64(iteration))
    h = lowbias32(h + np.uint64(k))
    return lowbias32(h + np.asarray(pixel, np.uint64))


def quantise(image, mask, sources=None):
    v = np.asarray(image, np.float32)
    fin = np.isfinite(v).all(-1)
    hole = np.asarray(mask, bool) | ~fin
    q = np.rint(np.clip(np.where(np.isfinite(v), v, np.float32(0)), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int32)
    q[hole] = 0
    bad = hole if sources is None else hole | ~np.asarray(sources, bool)
    return q, hole, bad


def box_any(a, P):
    """[h, w] bool: at inside centres, whether any pixel of the P x P patch is set (separable); False elsewhere."""
    h, w = a.shape
    r = P // 2
    out = np.zeros((h, w), bool)
    if h < P or w < P:
        return out
    row = np.zeros((h, w - 2 * r), bool)
    for d in range(P):
        row |= a[:, d:d + w - 2 * r]
    col = np.zeros((h - 2 * r, w - 2 * r), bool)
    for d in range(P):
        col |= row[d:d + h - 2 * r]
    out[r:h - r, r:w - r] = col
    return out


def make_level(img, hole, bad, P):
    h, w = hole.shape
    r = P // 2
    inside = np.zeros((h, w), bool)
    if h >= P and w >= P:
        inside[r:h - r, r:w - r] = True
    return {'img': img, 'hole': hole, 'bad': bad, 'T': box_any(hole, P), 'S': inside & ~box_any(bad, P) if inside.any() else inside,
            'h': h, 'w': w}


def down(lev, P):
    h2, w2 = lev['h'] // 2, lev['w'] // 2
    blk = lambda a: a[:2 * h2, :2 * w2].reshape((h2, 2, w2, 2) + a.shape[2:])
    known = ~blk(lev['hole'])
    n = known.sum((1, 3)).astype(np.int32)
    s = (blk(lev['img']) * known[..., None]).sum((1, 3)).astype(np.int32)
    img = np.where(n[..., None] > 0, (2 * s + n[..., None]) // (2 * np.maximum(n, 1)[..., None]), 0).astype(np.int32)
    return make_level(img, n < 4, blk(lev['bad']).any((1, 3)), P)


def ssd(img, ty, tx, sy, sx, P):
    r = P // 2
    d = np.arange(-r, r + 1)
    a = img[(ty[:, None, None] + d[None, :, None]), (tx[:, None, None] + d[None, None, :])]
    b = img[(sy[:, None, None] + d[None, :, None]), (sx[:, None, None] + d[None, None, :])]
    return ((a - b) ** 2).sum((1, 2, 3)).astype(np.int64)


def vote(lev, nnf, P):
    h, w, r, img = lev['h'], lev['w'], P // 2, lev['img']
    hy, hx = np.nonzero(lev['hole'])
    acc, cnt = np.zeros((len(hy), 3), np.int32), np.zeros(len(hy), np.int32)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ty, tx = hy - dy, hx - dx
            ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            s = nnf[np.clip(ty, 0, h - 1) * w + np.clip(tx, 0, w - 1)]
            ok &= s >= 0
            s = np.where(ok, s, r * w + r)
            acc += np.where(ok[:, None], img[s // w + dy, s % w + dx], 0)
            cnt += ok
    if len(hy):
        img[hy, hx] = (2 * acc + cnt[:, None]) // (2 * cnt[:, None])


def initial(lev, l, parent, parent_nnf, P, seed):
    h, w, r = lev['h'], lev['w'], P // 2
    ty, tx = np.nonzero(lev['T'])
    pix = ty * w + tx
    sidx = np.flatnonzero(lev['S'])
    s = sidx[(hash5(seed, l, INIT, 0, pix) % np.uint64(len(sidx))).astype(np.int64)] if len(pix) else pix
    if parent is not None and len(pix):
        h2, w2 = parent['h'], parent['w']
        py, px = ty >> 1, tx >> 1
        ok = (py < h2) & (px < w2)
        ps = parent_nnf[np.minimum(py, h2 - 1) * w2 + np.minimum(px, w2 - 1)]
        ok &= ps >= 0
        ps = np.where(ok, ps, 0)
        sy = np.clip(2 * (ps // w2) + (ty & 1), r, h - 1 - r)
        sx = np.clip(2 * (ps % w2) + (tx & 1), r, w - 1 - r)
        ok &= lev['S'][sy, sx]
        s = np.where(ok, sy * w + sx, s)
    nnf = np.full(h * w, -1, np.int64)
    nnf[pix] = s
    return nnf


def search(lev, l, it, old, P, seed):
    h, w, r, img, S = lev['h'], lev['w'], P // 2, lev['img'], lev['S']
    ty, tx = np.nonzero(lev['T'])
    if not len(ty):
        return old.copy()
    pix = ty * w + tx
    cur = old[pix].copy()
    best = ssd(img, ty, tx, cur // w, cur % w, P)

    def consider(cy, cx, ok):
        nonlocal cur, best
        ok = ok & (cy >= r) & (cy <= h - 1 - r) & (cx >= r) & (cx <= w - 1 - r)
        cy, cx = np.clip(cy, r, h - 1 - r), np.clip(cx, r, w - 1 - r)
        ok &= S[cy, cx]
        d = ssd(img, ty, tx, cy, cx, P)
        better = ok & (d < best)
        cur = np.where(better, cy * w + cx, cur)
        best = np.where(better, d, best)

    for st in (1, 2, 4):
        for dy, dx in ((0, -st), (0, st), (-st, 0), (st, 0)):
            qy, qx = ty + dy, tx + dx
            ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            sq = old[np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)]
            ok &= sq >= 0
            consider(sq // w - dy, sq % w - dx, ok)
    R, k = max(h, w), 0
    while R >= 1:
        hs = hash5(seed, l, it, k, pix)
        ry = (hs & np.uint64(0xffff)).astype(np.int64) % (2 * R + 1) - R
        rx = (hs >> np.uint64(16)).astype(np.int64) % (2 * R + 1) - R
        consider(cur // w + ry, cur % w + rx, np.ones(len(pix), bool))
        R //= 2
        k += 1
    new = old.copy()
    new[pix] = cur
    return new


def geometric_levels(H, W, P, max_levels=None):
    L, h, w = 1, H, W
    while (max_levels is None or L < max_levels) and min(h, w) // 2 >= 4 * P:
        h, w, L = h // 2, w // 2, L + 1
    return L


def fill_image(image, mask, patch=7, rounds=3, iters=4, seed=0, sources=None, max_levels=None, trace=None):
    """One image.  Returns (filled [H, W, 3] fp32, nnf [H, W, 2] int32, dict(targets, sources, levels, energy, singular)).
    trace: a list that receives (level, 'initial' | 'vote' | 'search', nnf copy, image copy) after every step."""
    P = int(patch)
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    q, hole, bad = quantise(image, mask, sources)
    levels = [make_level(q, hole, bad, P)]
    info = {'targets': int(levels[0]['T'].sum()), 'sources': int(levels[0]['S'].sum()), 'levels': 0, 'energy': 0, 'singular': False}
    nnf_out = np.full((H, W, 2), -1, np.int32)
    if not levels[0]['S'].any():
        info['singular'] = True
        return image.copy(), nnf_out, info
    while len(levels) < geometric_levels(H, W, P, max_levels):
        nxt = down(levels[-1], P)
        if not nxt['S'].any():
            break
        levels.append(nxt)
    info['levels'] = len(levels)
    note = (lambda *a: trace.append((a[0], a[1], a[2].copy(), a[3]['img'].copy()))) if trace is not None else (lambda *a: None)
    nnf = None
    for l in range(len(levels) - 1, -1, -1):
        lev = levels[l]
        nnf = initial(lev, l, levels[l + 1] if l + 1 < len(levels) else None, nnf, P, seed)
        note(l, 'initial', nnf, lev)
        vote(lev, nnf, P)
        note(l, 'vote', nnf, lev)
        it = 0
        for _ in range(rounds):
            for _ in range(iters):
                nnf = search(lev, l, it, nnf, P, seed)
                note(l, 'search', nnf, lev)
                it += 1
            vote(lev, nnf, P)
            note(l, 'vote', nnf, lev)
    lev = levels[0]
    ty, tx = np.nonzero(lev['T'])
    s = nnf[ty * W + tx]
    info['energy'] = int(ssd(lev['img'], ty, tx, s // W, s % W, P).sum()) if len(ty) else 0
    nnf_out[ty, tx, 0], nnf_out[ty, tx, 1] = s // W, s % W
    out = image.copy()
    out[hole] = lev['img'][hole].astype(np.float32) / np.float32(255)
    return out, nnf_out, info


def fill(images, masks, patch=7, rounds=3, iters=4, seed=0, sources=None, max_levels=None):
    """The batch: (filled [N, H, W, 3], info) with info as ops.exemplar_fill's, nnf a numpy array."""
    images, masks = np.asarray(images, np.float32), np.asarray(masks, bool)
    N, H, W = masks.shape
    out, nnf = np.empty_like(images), np.empty((N, H, W, 2), np.int32)
    keys = ('targets', 'sources', 'levels', 'energy', 'singular')
    rows = []
    for n in range(N):
        out[n], nnf[n], i = fill_image(images[n], masks[n], patch, rounds, iters, seed, None if sources is None else sources[n], max_levels)
        rows.append(i)
    info = {k: np.array([r[k] for r in rows], bool if k == 'singular' else np.int64) for k in keys}
    info['nnf'] = nnf
    return out, info


def jacobi_harmonic(q, hole, sweeps=4000):
    """Plain Jacobi harmonic fill of [H, W, C] float64 inside `hole` (mirror boundary at the image border): the yardstick of the
    periodic-recovery test."""
    u = np.where(hole[..., None], q[~hole].mean(0), q).astype(np.float64)
    H, W = hole.shape
    deg = np.full((H, W), 4.0)
    deg[0] -= 1
    deg[-1] -= 1
    deg[:, 0] -= 1
    deg[:, -1] -= 1
    for _ in range(sweeps):
        s = np.zeros_like(u)
        s[1:] += u[:-1]
        s[:-1] += u[1:]
        s[:, 1:] += u[:, :-1]
        s[:, :-1] += u[:, 1:]
        u = np.where(hole[..., None], s / deg[..., None], u)
    return u


def periodic_textures(H=72, W=96):
    """The three exactly periodic fixtures of the issue as fp32 images in 0..1 (k / 255): an 8 x 8 random tile, a 6-pixel
    checker, 3-channel stripes (periods 4, 6, 8 along x, y, x + y)."""
    y, x = np.mgrid[0:H, 0:W]
    tile = np.random.RandomState(11).randint(0, 256, (8, 8, 3))
    a = tile[y % 8, x % 8]
    c = (((y // 6) + (x // 6)) % 2)[..., None] * np.array([200, 180, 160]) + 30
    s = np.stack([(x % 4) * 60 + 20, (y % 6) * 40 + 10, ((x + y) % 8) * 30 + 15], -1)
    return [(t.astype(np.float32) / np.float32(255)) for t in (a, c, s)]


def periodic_holes(H=72, W=96):
    m = np.zeros((H, W), bool)
    m[25:45, 30:58] = True
    m[10:14, 70:90] = True
    return m
