"""Exemplar-based inpainting without a GPU: the restatement (tests/exemplar_numpy.py) against an independent per-pixel
Python-loop statement, the recovery of exactly periodic textures against a plain Jacobi harmonic fill, determinism, the known
pixels, the argument checks of the mvip_exemplar_* entry points with NULL operands, the refusals of ops.exemplar_fill,
prepare.inpaint_views and propagate_reference(fill=...), and the tools' --help."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exemplar_numpy as R                               # noqa: E402

from mvip_nerf_amd import _lib, ops, prepare             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'scene1_small.npz')
OK, EINVAL = 0, -1
P0 = None            # NULL
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the definition once more, one pixel at a time in Python integers ------------------------------------------------------------------

def mix(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def rnd(seed, level, iteration, k, pixel):
    h = mix(seed ^ 0x9e3779b9)
    for v in (level, iteration, k, pixel):
        h = mix(h + v)
    return h


def loop_sets(lev, P):
    h, w, r = lev['h'], lev['w'], P // 2
    lev['T'], lev['S'] = set(), []
    for y in range(r, h - r):
        for x in range(r, w - r):
            cells = [(y + a, x + b) for a in range(-r, r + 1) for b in range(-r, r + 1)]
            if any(lev['hole'][c] for c in cells):
                lev['T'].add((y, x))
            else:
                lev['S'].append((y, x))                  # row-major
    lev['Sset'] = set(lev['S'])


def loop_down(lev, P):
    h2, w2 = lev['h'] // 2, lev['w'] // 2
    out = {'h': h2, 'w': w2, 'img': {}, 'hole': {}}
    for y in range(h2):
        for x in range(w2):
            four = [(2 * y + a, 2 * x + b) for a in (0, 1) for b in (0, 1)]
            known = [c for c in four if not lev['hole'][c]]
            out['hole'][(y, x)] = len(known) < 4
            n = len(known)
            out['img'][(y, x)] = [(2 * sum(lev['img'][c][ch] for c in known) + n) // (2 * n) if n else 0 for ch in range(3)]
    loop_sets(out, P)
    return out


def loop_ssd(lev, t, s, P, stop=None):
    r, total = P // 2, 0
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            p, q = lev['img'][(t[0] + a, t[1] + b)], lev['img'][(s[0] + a, s[1] + b)]
            total += sum((p[c] - q[c]) ** 2 for c in range(3))
        if stop is not None and total >= stop:
            return total                                 # the early exit: it cannot win any more
    return total


def loop_vote(lev, nnf, P):
    r = P // 2
    new = {}
    for p, is_hole in lev['hole'].items():
        if not is_hole:
            continue
        vals = []
        for a in range(-r, r + 1):
            for b in range(-r, r + 1):
                t = (p[0] - a, p[1] - b)
                if t in nnf:
                    s = nnf[t]
                    vals.append(lev['img'][(s[0] + a, s[1] + b)])
        n = len(vals)
        new[p] = [(2 * sum(v[c] for v in vals) + n) // (2 * n) for c in range(3)]
    lev['img'].update(new)


def loops_fill(image, mask, P, rounds, iters, seed):
    """Returns the trace: [(level, nnf as an array [h, w] of y w + x or -1, image [h, w, 3])] after every step."""
    H, W = mask.shape
    r = P // 2
    lev = {'h': H, 'w': W, 'img': {}, 'hole': {}}
    for y in range(H):
        for x in range(W):
            v = image[y, x]
            hole = bool(mask[y, x]) or not all(np.isfinite(c) for c in v)
            lev['hole'][(y, x)] = hole
            lev['img'][(y, x)] = [0, 0, 0] if hole else [int(np.rint(np.float32(min(max(np.float32(c), np.float32(0)), np.float32(1))) * np.float32(255))) for c in v]
    loop_sets(lev, P)
    levels = [lev]
    while min(levels[-1]['h'], levels[-1]['w']) // 2 >= 4 * P:
        nxt = loop_down(levels[-1], P)
        if not nxt['S']:
            break
        levels.append(nxt)
    trace, nnf = [], None

    def note(l, lev, nnf):
        a = np.full((lev['h'], lev['w']), -1, np.int64)
        for t, s in nnf.items():
            a[t] = s[0] * lev['w'] + s[1]
        trace.append((l, a.reshape(-1), np.array([[lev['img'][(y, x)] for x in range(lev['w'])] for y in range(lev['h'])])))

    for l in range(len(levels) - 1, -1, -1):
        lev = levels[l]
        h, w = lev['h'], lev['w']
        parent, new = nnf, {}
        for t in sorted(lev['T']):
            s = None
            if parent is not None:
                pt = (t[0] >> 1, t[1] >> 1)
                if pt in parent:
                    ps = parent[pt]
                    c = (min(max(2 * ps[0] + (t[0] & 1), r), h - 1 - r), min(max(2 * ps[1] + (t[1] & 1), r), w - 1 - r))
                    if c in lev['Sset']:
                        s = c
            if s is None:
                s = lev['S'][rnd(seed, l, 0xffffffff, 0, t[0] * w + t[1]) % len(lev['S'])]
            new[t] = s
        nnf = new
        note(l, lev, nnf)
        loop_vote(lev, nnf, P)
        note(l, lev, nnf)
        it = 0
        for _ in range(rounds):
            for _ in range(iters):
                new = {}
                for t in lev['T']:
                    cur = nnf[t]
                    best = loop_ssd(lev, t, cur, P)
                    cands = []
                    for st in (1, 2, 4):
                        for d in ((0, -st), (0, st), (-st, 0), (st, 0)):
                            q = (t[0] + d[0], t[1] + d[1])
                            if q in nnf:
                                cands.append((nnf[q][0] - d[0], nnf[q][1] - d[1]))
                    for c in cands:
                        if c in lev['Sset']:
                            e = loop_ssd(lev, t, c, P, best)
                            if e < best:
                                cur, best = c, e
                    Rr, k = max(h, w), 0
                    while Rr >= 1:
                        hs = rnd(seed, l, it, k, t[0] * w + t[1])
                        c = (cur[0] + (hs & 0xffff) % (2 * Rr + 1) - Rr, cur[1] + (hs >> 16) % (2 * Rr + 1) - Rr)
                        if c in lev['Sset']:
                            e = loop_ssd(lev, t, c, P, best)
                            if e < best:
                                cur, best = c, e
                        Rr //= 2
                        k += 1
                    new[t] = cur
                nnf = new
                note(l, lev, nnf)
                it += 1
            loop_vote(lev, nnf, P)
            note(l, lev, nnf)
    return trace


def small_picture(H, W, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x % 5) * 0.2, (y % 4) * 0.25, ((x + 2 * y) % 7) / 7.0], -1) + rs.uniform(-0.08, 0.08, (H, W, 3))
    img = img.astype(np.float32)
    img[0, 3] = (-0.5, 1.5, 0.5)
    return img


@pytest.mark.parametrize('H,W,P,boxes', [(20, 24, 5, ((7, 12, 9, 15),)), (20, 24, 5, ((0, 4, 0, 5),)), (20, 24, 5, ((7, 12, 9, 15), (15, 20, 19, 24))),
                                         (24, 28, 3, ((8, 14, 10, 17), (0, 3, 24, 28)))])
def test_restatement_equals_per_pixel_loops(H, W, P, boxes):
    img = small_picture(H, W, H + P)
    m = np.zeros((H, W), bool)
    for y0, y1, x0, x1 in boxes:
        m[y0:y1, x0:x1] = True
    img[H - 2, 2, 1] = np.nan                            # joins the hole
    trace = []
    out, nnf, info = R.fill_image(img, m, P, rounds=2, iters=2, seed=4, trace=trace)
    want = loops_fill(img, m, P, 2, 2, 4)
    assert info['levels'] == (2 if P == 3 else 1) and len(trace) == len(want) == info['levels'] * (2 + 2 * 3)
    for (l, _, a, b), (wl, wa, wb) in zip(trace, want):
        assert l == wl and np.array_equal(a, wa) and np.array_equal(b, wb), l
    assert info['targets'] == (want[-1][1] >= 0).sum() == (nnf[..., 0] >= 0).sum()
    assert np.array_equal(bits(out)[~(m | ~np.isfinite(img).all(-1))], bits(img)[~(m | ~np.isfinite(img).all(-1))])
    hole = m | ~np.isfinite(img).all(-1)
    assert np.array_equal(out[hole], want[-1][2][hole].astype(np.float32) / np.float32(255))


# ---- what the fill is for ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('which', [0, 1, 2])
def test_periodic_textures_are_recovered(which):
    """72 x 96, two holes, patch 7, seeds 1..3: the in-hole RMS (in 1 / 255) must be at most half of a plain Jacobi harmonic
    fill's.  (The restatement gives exactly 0 against 69 to 84.)"""
    t, m = R.periodic_textures()[which], R.periodic_holes()
    q = np.rint(t * 255).astype(np.float64)
    harmonic = R.jacobi_harmonic(q, m, 1500)
    e_h = float(np.sqrt(((harmonic - q)[m] ** 2).mean()))
    for seed in (1, 2, 3):
        out, _, info = R.fill_image(t, m, 7, seed=seed)
        e = float(np.sqrt(((out.astype(np.float64) * 255 - q)[m] ** 2).mean()))
        print(f'texture {which} seed {seed}: exemplar RMS {e:.3f}, harmonic {e_h:.3f}, levels {info["levels"]}, energy {info["energy"]}')
        assert info['levels'] == 2 and e <= 0.5 * e_h


def real_case():
    z = np.load(FIXTURE, allow_pickle=False)
    img = z['images'][0, 0:64, 0:96].astype(np.float32) / np.float32(255.)
    m = np.zeros((64, 96), bool)
    m[10:34, 20:52] = True
    return img, m | z['masks'][0, 0:64, 0:96].astype(bool)


def test_determinism_and_known_pixels():
    img, m = real_case()
    a, b, c = (R.fill_image(img, m, 7, seed=s) for s in (1, 1, 2))
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert not np.array_equal(a[1], c[1])                # another seed, another field
    assert a[2]['levels'] == 2 and a[2]['targets'] > m.sum() and a[2]['energy'] > 0
    for out in (a[0], c[0]):
        assert np.array_equal(bits(out)[~m], bits(img)[~m])
        inside = out[m]
        assert np.array_equal(inside, np.rint(inside * 255).astype(np.float32) / np.float32(255)) and inside.std() > 0.02
    # the batch form, a singular image and an empty mask
    rim = np.ones_like(m)
    rim[:3], rim[-3:], rim[:, :3], rim[:, -3:] = False, False, False, False
    out, info = R.fill(np.stack([img, img, img]), np.stack([m, rim, np.zeros_like(m)]), seed=1)
    assert info['singular'].tolist() == [False, True, False] and info['levels'].tolist() == [2, 0, 2] and info['targets'][2] == 0
    assert np.array_equal(bits(out[0]), bits(a[0])) and np.array_equal(bits(out[1:]), bits(np.stack([img, img]))) and (info['nnf'][1:] == -1).all()
    assert R.geometric_levels(29, 29, 7) == 1 and R.geometric_levels(120, 136, 7) == 3 and R.geometric_levels(120, 136, 7, 2) == 2
    assert R.geometric_levels(72, 96, 7) == 2 and R.geometric_levels(48, 64, 7) == 1


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------

def test_entry_point_argument_checks():
    raw = lambda name, *a: getattr(_lib.load(), name)(*a)
    for name, n in (('mvip_exemplar_levels', 4), ('mvip_exemplar_meta_words', 1), ('mvip_exemplar_workspace_bytes', 5),
                    ('mvip_exemplar_setup', 11), ('mvip_exemplar_lists', 10), ('mvip_exemplar_level', 15), ('mvip_exemplar_finish', 13)):
        assert name in _lib.DECLARED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == n
    assert _lib.ABI_VERSION == 5
    assert raw('mvip_exemplar_levels', 29, 29, 7, 0) == 1 and raw('mvip_exemplar_levels', 120, 136, 7, 0) == 3
    assert raw('mvip_exemplar_levels', 120, 136, 7, 2) == 2 and raw('mvip_exemplar_levels', 378, 504, 7, 0) == 4
    assert raw('mvip_exemplar_levels', 16384, 16384, 3, 0) == 8
    for H, W, P, cap in ((6, 29, 7, 0), (29, 6, 7, 0), (29, 29, 6, 0), (29, 29, 11, 0), (29, 29, 1, 0), (16385, 29, 7, 0), (0, 0, 7, 0), (29, 29, 7, -1)):
        assert raw('mvip_exemplar_levels', H, W, P, cap) == -1, (H, W, P, cap)
    assert raw('mvip_exemplar_meta_words', 0) == 96 and raw('mvip_exemplar_meta_words', 3) == 96 + 3 * 32
    assert raw('mvip_exemplar_meta_words', -1) == -1 and raw('mvip_exemplar_meta_words', 1 << 40) == -1
    assert raw('mvip_exemplar_workspace_bytes', 0, 37, 53, 7, 1) == 0 and raw('mvip_exemplar_workspace_bytes', 2, 37, 53, 7, 1) >= 2 * 37 * 53 * 14
    assert raw('mvip_exemplar_workspace_bytes', 2, 37, 53, 7, 2) == -1           # more levels than the geometry gives
    assert raw('mvip_exemplar_workspace_bytes', -1, 37, 53, 7, 1) == -1 and raw('mvip_exemplar_workspace_bytes', 1 << 40, 37, 53, 7, 1) == -1
    assert raw('mvip_exemplar_workspace_bytes', 4, 16384, 16384, 7, 1) == -1     # beyond the index range

    def each(N, H, W, P, L, level=0, nt=5, nh=5, rounds=3, iters=4, cap=10):
        return (raw('mvip_exemplar_setup', P0, P0, P0, N, H, W, P, L, P0, P0, P0),
                raw('mvip_exemplar_lists', N, H, W, P, L, P0, P0, P0, cap, P0),
                raw('mvip_exemplar_level', N, H, W, P, L, level, nt, nh, rounds, iters, 0, P0, P0, P0, P0),
                raw('mvip_exemplar_finish', P0, N, H, W, P, L, rounds, iters, P0, P0, P0, P0, P0))
    for N, H, W, P, L in ((-1, 37, 53, 7, 1), (2, 6, 53, 7, 1), (2, 37, 53, 4, 1), (2, 37, 53, 11, 1), (2, 37, 53, 7, 0), (2, 37, 53, 7, 2),
                          (2, 16385, 53, 7, 1), (0, 6, 53, 7, 1), (1 << 40, 37, 53, 7, 1)):
        assert each(N, H, W, P, L) == (EINVAL,) * 4, (N, H, W, P, L)            # a bad shape, also with no image
    assert each(0, 37, 53, 7, 1, nt=0, nh=0, cap=0) == (OK,) * 4                                    # no image: nothing launched
    assert each(2, 37, 53, 7, 1) == (EINVAL,) * 4                                # NULL operands
    assert each(2, 120, 136, 7, 3, level=2) == (EINVAL,) * 4
    level = lambda **kw: each(2, 37, 53, 7, 1, **kw)[2]
    assert level(level=1) == EINVAL and level(level=-1) == EINVAL and level(rounds=-1) == EINVAL and level(iters=-1) == EINVAL
    assert level(nt=-1) == EINVAL and level(nh=-1) == EINVAL and level(nt=2 * 37 * 53 + 1) == EINVAL and level(nt=0) == EINVAL
    assert level(nt=0, nh=0) == OK                                               # no target: nothing launched
    assert each(2, 37, 53, 7, 1, cap=-1)[1] == EINVAL and each(2, 37, 53, 7, 1, rounds=-1)[3] == EINVAL


def test_wrappers_refuse_bad_arguments():
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    good = lambda: dict(images=z(2, 12, 14, 3), masks=z(2, 12, 14, dtype=torch.bool))

    def check(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.exemplar_fill(**dict(good(), **kw))
    check('GPU')                                                                 # CPU tensors
    check('GPU', images=np.zeros((2, 12, 14, 3), np.float32))
    check('images', images=z(2, 12, 14, 3, dtype=torch.float64))
    check('images', images=z(2, 12, 14))
    check('images', images=z(2, 12, 14, 4))
    check('bool', masks=z(2, 12, 14, dtype=torch.uint8))
    check('masks', masks=z(2, 12, 15, dtype=torch.bool))
    check('sources', sources=z(2, 12, 15, dtype=torch.bool))
    check('bool', sources=z(2, 12, 14))
    check('patch', patch=6)
    check('patch', patch=11)
    check('patch', patch=1)
    check('smaller', patch=9, images=z(2, 8, 14, 3), masks=z(2, 8, 14, dtype=torch.bool))
    check('rounds', rounds=-1)
    check('iters', iters=-1)
    check('max_levels', max_levels=0)
    check('seed', seed=-1)
    p = inspect.signature(ops.exemplar_fill).parameters
    assert list(p) == ['images', 'masks', 'patch', 'rounds', 'iters', 'seed', 'sources', 'max_levels']
    assert [p[k].default for k in list(p)[2:]] == [7, 3, 4, 0, None, None]

    img, m, d, poses = np.zeros((4, 12, 14, 3), np.float32), np.zeros((4, 12, 14), bool), np.ones((4, 12, 14), np.float32), np.zeros((4, 3, 4), np.float32)
    for fill in ('lama', 'Exemplar', ''):
        with pytest.raises(ValueError, match='fill'):
            prepare.propagate_reference(img, m, d, poses, 9.0, [0], fill=fill)
    for fill in ('exemplar', 'harmonic', 'none', True, False):                   # the known ones pass on to the other checks
        with pytest.raises(ValueError, match='ref_views'):
            prepare.propagate_reference(img, m, d, poses, 9.0, [], fill=fill)
    assert inspect.signature(prepare.propagate_reference).parameters['fill'].default is True
    p = inspect.signature(prepare.inpaint_views).parameters
    assert list(p)[:4] == ['images', 'masks', 'views', 'method'] and p['method'].default == 'exemplar'
    for match, a, kw in (('method', (img, m, [0]), {'method': 'lama'}), ('images', (img[..., 0], m, [0]), {}), ('masks', (img, m[:3], [0]), {}),
                         ('views', (img, m, []), {}), ('views', (img, m, [4]), {})):
        with pytest.raises(ValueError, match=match):
            prepare.inpaint_views(*a, **kw)


def test_tools_help():
    for tool, opts in (('propagate_reference.py', ('--inpaint', '--fill', 'exemplar', 'harmonic', '--ref-image')),
                       ('exemplar_bench.py', ('--out', '--repeats'))):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool), '--help'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for opt in opts:
            assert opt in r.stdout, (tool, opt)
