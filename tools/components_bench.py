"""Connected-components timings (profiles/components.json): the pack, label and select passes of csrc/components.hip at
128^3, 256^3 and 512^3 on a thresholded gyroid (one large component) and on the seeded p = 0.34 random field (many small
ones), HIP-event times of steady-state repeats after a warm-up, on preallocated buffers; the API call (allocation and the
one read-back included); scipy.ndimage.label on the host for the same fields where scipy imports; and the yardstick: the
fp32 sigma query of the 256^3 lattice (mesh.density_grid, 8x256 MLP), measured in the same run.

Bytes each pass must move (N elements): pack reads 4 N and writes N / 8.  label = init (N / 8 read, 4 N parent written) +
union (N / 8 + 4 N read; the parent words the finds and the atomics touch beyond that are not counted) + compress (4 N
read, up to 4 N written) + rank and assign (4 N parent read each, 4 N labels written): 28.25 N.  select reads 4 N and
writes N / 8.

--scene1 measures the feature on the scene-1 fixture instead (profiles/components_scene1.json): the field of the
1,500-iteration recipe (tools/render_occupancy_ab.py::train_scene1); the mesh at tools/extract_mesh.py's defaults
(resolution 256, threshold 10; its default box and the cameras' frustum box) before and after largest = 1; the region
lifted from view 0 at tools/propagate_masks.py's defaults, its cells and the mean IoU over the other 29 views with and
without keep_components(largest=1).

  python tools/components_bench.py [--out profile_out/components.json] [--sizes 128 256 512] [--commit HASH]
  python tools/components_bench.py --scene1 [--out profile_out/components_scene1.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import _lib, mesh, ops, run                       # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.extract_mesh import model_args                            # noqa: E402
from tools.mesh_bench import HBM_BYTES_PER_S, event_ms, gyroid       # noqa: E402

I32 = torch.int32


def fields(n, dev):
    yield 'gyroid, 4 periods, >= 1.5', gyroid(n, dev), 1.5
    rs = np.random.RandomState(7)
    yield 'RandomState(7).rand < 0.34', torch.from_numpy((rs.rand(n, n, n) < 0.34).astype(np.float32)).to(dev), 0.5


def row(n, name, values, thr, connectivity, dev, host):
    N = n ** 3
    words = ops.grid_pack(values, thr)
    labels, sizes, first = ops.grid_components(words, (n, n, n), connectivity)
    nc = int(sizes.shape[0])
    G = _lib.load().mvip_components_groups(n, n, n)
    parent = torch.empty(N, device=dev, dtype=I32)
    wg = torch.empty(G, device=dev, dtype=I32)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    keep = torch.zeros(nc + 1, device=dev, dtype=torch.uint8)
    keep[1 + int(sizes.argmax())] = 1
    out_words = torch.empty_like(words)

    def pack():
        call('mvip_components_pack', ptr(values), N, thr, ptr(out_words, I32), stream())

    def label():
        call('mvip_components_label', ptr(words, I32), n, n, n, connectivity, ptr(parent, I32), ptr(wg, I32),
             ptr(total, torch.int64), stream())
        call('mvip_components_rank', ptr(parent, I32), n, n, n, ptr(wg, I32), nc, ptr(labels, I32), ptr(sizes, I32),
             ptr(first, I32), stream())

    def select():
        call('mvip_components_select', ptr(labels, I32), N, ptr(keep, torch.uint8), nc, ptr(out_words, I32), stream())

    t_pack, _ = event_ms(pack)
    t_label, reps = event_ms(label)
    assert int(total.cpu()) == nc
    t_select, _ = event_ms(select)
    t_api, _ = event_ms(lambda: ops.grid_components(words, (n, n, n), connectivity), warmup=1, reps=3)
    nbytes = {'pack': 4 * N + N // 8, 'label': 28 * N + N // 4, 'select': 4 * N + N // 8}
    frac = lambda b, ms: round(b / (ms * 1e-3) / HBM_BYTES_PER_S, 3)
    r = {'grid': [n, n, n], 'field': name, 'connectivity': connectivity, 'set_share': round(float(sizes.sum()) / N, 4),
         'components': nc, 'largest': int(sizes.max()) if nc else 0,
         'ms_pack': round(t_pack, 4), 'ms_label': round(t_label, 4), 'ms_label_reps': [round(t, 4) for t in reps],
         'ms_select': round(t_select, 4), 'ms_label_plus_select': round(t_label + t_select, 4),
         'ms_api_grid_components': round(t_api, 4), 'compulsory_bytes': nbytes,
         'fraction_of_6.3_TB_s': {'pack': frac(nbytes['pack'], t_pack), 'label': frac(nbytes['label'], t_label),
                                  'select': frac(nbytes['select'], t_select)},
         'note': 'labels exceed the 256 MiB Infinity Cache: an HBM figure' if 4 * N > 256 * 2 ** 20
         else 'labels fit the 256 MiB Infinity Cache: not an HBM figure'}
    if host:
        try:
            from scipy import ndimage
        except ImportError:
            r['ms_scipy_label_host'] = None
        else:
            bits = (values >= thr).cpu().numpy()
            t0 = time.perf_counter()
            _, m = ndimage.label(bits, ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3))
            r['ms_scipy_label_host'] = round((time.perf_counter() - t0) * 1e3, 1)
            assert m == nc, (m, nc)
    return r


def sigma_query_ms(n, dev):
    from oracle.weights import seeded_state_dict
    _, kw, _, _, _ = run.create_nerf(model_args(64), device=dev)
    kw['network_fine'].load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(1).items()})
    kw['network_fine'].inference_precision = 0
    t, reps = event_ms(lambda: mesh.density_grid(kw, (-1, -1, -1), (1, 1, 1), n), warmup=1, reps=3)
    return round(t, 2), [round(x, 2) for x in reps]


def scene1(dev, iters):
    from mvip_nerf_amd.region import Region, propagate_masks
    from tools import render_occupancy_ab as T
    from tools.propagate_masks import iou
    scene = T.train_scene1(dev, iters)
    te, hwf, poses, near, far = scene['te'], (scene['H'], scene['W'], scene['focal']), scene['poses'], scene['near'], scene['far']
    out = {'fixture': 'tests/golden/scene1_small.npz', 'iterations': iters, 'mesh': [], 'region': []}
    thr, res = 10.0, 256
    for name, (lo, hi) in (('tools/extract_mesh.py default box', ((-1.0,) * 3, (1.0,) * 3)), ('frustum box', T.scene_bounds(scene))):
        grid = mesh.density_grid(te, lo, hi, res)
        sizes = ops.grid_components(ops.grid_pack(grid, thr), grid.shape)[1]
        rec = {'box': name, 'box_min': [float(v) for v in lo], 'box_max': [float(v) for v in hi], 'resolution': res,
               'threshold': thr, 'inside_points': int(sizes.sum()), 'components': int(sizes.shape[0]),
               'largest_component_points': int(sizes.max()) if sizes.shape[0] else 0,
               'components_of_one_point': int((sizes == 1).sum())}
        v, f, _ = mesh.marching_cubes(grid, thr, lo, hi)
        rec['vertices'], rec['triangles'] = int(v.shape[0]), int(f.shape[0])
        if sizes.shape[0]:
            v, f, _ = mesh.marching_cubes(mesh.remove_floaters(grid, thr, largest=1), thr, lo, hi)
            rec['vertices_keep_largest_1'], rec['triangles_keep_largest_1'] = int(v.shape[0]), int(f.shape[0])
        out['mesh'].append(rec)
        del grid
    masks = np.load(T.FIXTURE)['masks'].astype(bool)
    lifted = Region.from_masks(te, hwf, poses[[0]], torch.from_numpy(masks[[0]]).to(dev), near, far, cells=64, dilate=1)
    sizes = lifted.components()[1]
    for name, region in (('as lifted', lifted), ('keep_components(largest=1)', lifted.keep_components(largest=1))):
        hard = propagate_masks(te, hwf, poses, region, near, far, 0.5)[1].cpu().numpy()
        ious = [iou(hard[v], masks[v]) for v in range(1, len(masks))]
        out['region'].append({'region': name, 'annotated': [0], 'cells': region.count(), 'components': int(region.components()[1].shape[0]),
                              'mean_iou_other_views': float(np.mean(ious)), 'min_iou_other_views': float(np.min(ious)),
                              'iou_annotated_view': iou(hard[0], masks[0])})
    out['region_component_sizes_largest_10'] = sorted((int(x) for x in sizes.cpu()), reverse=True)[:10]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--scene1', action='store_true')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --scene1')
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--no-host', action='store_true', help='skip the scipy baseline')
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'components_scene1.json' if a.scene1 else 'components.json')
    if a.scene1:
        out = dict(scene1(dev, a.iters), commit=a.commit, device=torch.cuda.get_device_name(0))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return 0
    rows = []
    for n in a.sizes:
        for name, values, thr in fields(n, dev):
            for conn in (6, 26):
                rows.append(row(n, name, values, thr, conn, dev, host=not a.no_host and conn == 6))
            del values
    t_query, reps = sigma_query_ms(256, dev)
    worst = max(r['ms_label_plus_select'] for r in rows if r['grid'][0] == 256) if 256 in a.sizes else None
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'passes': rows,
           'yardstick': {'ms_sigma_query_256_fp32': t_query, 'ms_sigma_query_reps': reps,
                         'ms_label_plus_select_256_worst_row': worst,
                         'label_plus_select_below_query': None if worst is None else bool(worst < t_query)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
