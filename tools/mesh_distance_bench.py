"""Mesh-to-mesh distance timings and the clean-up error table (profiles/mesh_distance.json, profiles/mesh_distance_cleanup.json;
csrc/mesh_distance.hip) on the marching-cubes mesh of the 4-period gyroid of tools/mesh_ops_bench.py (256^3: 2.5 M triangles).

Timings (--what timing): the face grid's build (the API call ops.mesh_face_grid with its two read-backs, and its cells / pairs /
longest list); then, for the mesh clustered at 2 / 4 / 8 lattice steps, the query of that mesh's samples (--samples^2 per face,
face-major) against the full mesh: HIP-event time of ops.mesh_closest_point with a given grid (one launch and its three output
allocations), point-face tests per query and the lane utilisation of the face loop (tests / (64 x the busiest lane's tests, summed
over the waves)) from the counting variant, and the achieved fp64 rate at FLOPS_PER_TEST nominal
operations per test against the vector fp64 peak.  The same queries in a random order measure what the face-major order is worth
(neighbouring lanes walking the same cells).  The median of 5 windows after a warm-up.

The table (--what cleanup): for 5 / 10 / 20 Taubin iterations and for clustering at 2 / 4 / 8 lattice steps in both placements,
Chamfer distance, sampled Hausdorff distance and normal consistency of the cleaned mesh to the input, in units of the lattice
step (evaluate.mesh_distance_metrics); with --scene1 also the sigma = 10 mesh against the TSDF mesh of the scene-1 fixture field
(trained here, --iters iterations), whole and with the unseen faces dropped.  A record, not a gate.

  python tools/mesh_distance_bench.py [--what timing cleanup] [--scene1 [--iters 1500]] [--size 256] [--samples 2]
         [--out-dir profile_out] [--commit HASH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import evaluate, mesh, ops                        # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
# one point-triangle test with the interior candidate taken: 12 edge differences, the normal 9 + 5, three edge functions 3 x (3 + 9
# + 5), s 5, d2 and q 9, three segments of 28 -- a division counted as one operation
FLOPS_PER_TEST = 175
# vector (non-matrix) fp64 peak of the MI355X data sheet
PEAK_FP64_VECTOR_TFLOPS = 78.6


def timing(v, f, n, samples, dev):
    h = 2.0 / (n - 1)
    out = {}

    def build():
        out['g'] = ops.mesh_face_grid(v, f)
    t_grid, reps = event_ms(build, warmup=1, reps=5)
    g = out['g']
    lengths = g.cell_offsets[1:] - g.cell_offsets[:-1]
    r = {'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]), 'cells': list(g.cells), 'pairs': g.n_pairs,
         'pairs_per_face': round(g.n_pairs / f.shape[0], 3), 'longest_cell_list': int(lengths.max()),
         'share_of_cells_occupied': round(float((lengths > 0).float().mean()), 4), 'ms_api_mesh_face_grid': round(t_grid, 4),
         'ms_reps': [round(t, 4) for t in reps], 'queries': []}
    for steps in (2, 4, 8):
        cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, steps * h, 'quadric')
        pts = ops.mesh_sample_faces(cv, cf, samples)[0]
        N = int(pts.shape[0])
        shuffled = pts[torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(0))].contiguous()
        t_q, reps_q = event_ms(lambda: ops.mesh_closest_point(pts, v, f, grid=g))
        t_s, _ = event_ms(lambda: ops.mesh_closest_point(shuffled, v, f, grid=g))
        t_c, _ = event_ms(lambda: ops.mesh_closest_point(pts, v, f, grid=g, return_stats=True))
        face, _, dist, stats = ops.mesh_closest_point(pts, v, f, grid=g, return_stats=True)
        tests, slots = (int(x) for x in stats.cpu())
        tflops = tests * FLOPS_PER_TEST / (t_q * 1e-3) / 1e12
        r['queries'].append({'lattice_steps': steps, 'query_triangles': int(cf.shape[0]), 'queries': N, 'ms_query': round(t_q, 4),
                             'ms_reps': [round(t, 4) for t in reps_q], 'ms_query_random_order': round(t_s, 4),
                             'ms_query_counting_variant': round(t_c, 4), 'queries_per_second': round(N / (t_q * 1e-3)),
                             'point_face_tests_per_query': round(tests / N, 2),
                             'lane_utilisation_of_the_face_loop': round(tests / slots, 4), 'tflops_fp64_nominal': round(tflops, 3),
                             'share_of_vector_fp64_peak': round(tflops / PEAK_FP64_VECTOR_TFLOPS, 4),
                             'max_distance_in_steps': round(float(dist.max()) / h, 4)})
    return r


def cleanup(v, f, n, samples):
    h = 2.0 / (n - 1)
    first = mesh.Mesh(v, f, None, None)
    rows = []

    def row(what, m):
        rep = evaluate.mesh_distance_metrics(m, first, samples=samples, thresholds=(0.5 * h, h))
        rows.append({'clean_up': what, 'triangles': int(m.faces.shape[0]), 'chamfer_in_steps': round(rep['chamfer'] / h, 5),
                     'hausdorff_in_steps': round(rep['hausdorff'] / h, 5), 'normal_consistency': round(rep['normal_consistency'], 5),
                     'mean_to_input_in_steps': round(rep['a_to_b']['mean'] / h, 5), 'mean_from_input_in_steps': round(rep['b_to_a']['mean'] / h, 5),
                     'max_to_input_in_steps': round(rep['a_to_b']['max'] / h, 5), 'max_from_input_in_steps': round(rep['b_to_a']['max'] / h, 5),
                     'rms_to_input_in_steps': round(rep['a_to_b']['rms'] / h, 5), 'rms_from_input_in_steps': round(rep['b_to_a']['rms'] / h, 5),
                     'fscore_half_step': round(rep['fscore'][0], 5), 'fscore_one_step': round(rep['fscore'][1], 5)})
    for iters in (5, 10, 20):
        row(f'{iters} Taubin iterations', mesh.Mesh(ops.mesh_smooth(v, f, iters), f, None, None))
    for steps in (2, 4, 8):
        for placement in ('quadric', 'mean'):
            cv, cf, _, _ = ops.mesh_cluster(v, f, None, None, steps * h, placement)
            row(f'clustering at {steps} lattice steps ({placement})', mesh.Mesh(cv, cf, None, None))
    return {'vertices': int(v.shape[0]), 'triangles': int(f.shape[0]), 'samples_per_face': samples * samples, 'lattice_step': h, 'rows': rows}


def scene1(dev, iters, resolution, samples):
    """--scene1: the sigma = 10 mesh against the TSDF mesh of the trained scene-1 fixture field, whole and with the faces no
    training view sees dropped (the sigma mesh is mostly interior sheets), in units of the largest lattice step."""
    import numpy as np
    from mvip_nerf_amd import prepare
    from tools import propagate_masks as P
    te, hwf, poses, _, _, _, near, far, source = P.fixture_scene(dev, iters)
    poses = torch.as_tensor(poses).to(dev)[:, :3, :4].contiguous().float()
    lo32, hi32 = mesh._bounds(*mesh.frustum_bounds(poses, hwf, near, far))
    h = max(float((hi32[k] - lo32[k]) / np.float32(resolution - 1)) for k in range(3))
    disp = prepare.render_disparities(te, hwf, poses, near, far)
    v, f, n = mesh.marching_cubes(mesh.density_grid(te, lo32, hi32, resolution), 10.0, lo32, hi32)
    sigma, tsdf = mesh.Mesh(v, f, n, None), mesh.fuse_depths(disp, poses, float(hwf[2]), lo32, hi32, resolution)
    rows = []
    for what, a, b in (('sigma mesh against TSDF mesh', sigma, tsdf),
                       ('the same, faces no view sees dropped from both', mesh.keep_faces(sigma, mesh.visible_faces(sigma, hwf, poses)),
                        mesh.keep_faces(tsdf, mesh.visible_faces(tsdf, hwf, poses)))):
        rep = evaluate.mesh_distance_metrics(a, b, samples=samples, thresholds=(h, 2 * h))
        rows.append({'pair': what, 'triangles': [int(a.faces.shape[0]), int(b.faces.shape[0])], 'chamfer_in_steps': round(rep['chamfer'] / h, 4),
                     'hausdorff_in_steps': round(rep['hausdorff'] / h, 4), 'normal_consistency': round(rep['normal_consistency'], 4),
                     'mean_sigma_to_tsdf_in_steps': round(rep['a_to_b']['mean'] / h, 4), 'mean_tsdf_to_sigma_in_steps': round(rep['b_to_a']['mean'] / h, 4),
                     'precision_recall_fscore_one_step': [round(rep[k][0], 4) for k in ('precision', 'recall', 'fscore')],
                     'precision_recall_fscore_two_steps': [round(rep[k][1], 4) for k in ('precision', 'recall', 'fscore')]})
    return {'source': source, 'resolution': resolution, 'lattice_step': h, 'threshold': 10.0, 'samples_per_face': samples * samples, 'rows': rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', nargs='+', choices=('timing', 'cleanup'), default=['timing', 'cleanup'])
    ap.add_argument('--scene1', action='store_true', help='cleanup: also the sigma mesh against the TSDF mesh of the scene-1 fixture field')
    ap.add_argument('--iters', type=int, default=1500, help='training iterations of --scene1')
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--samples', type=int, default=2)
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profile_out'))
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    v, f, _ = mesh.marching_cubes(gyroid(a.size, dev), 1.5, LO, HI)
    os.makedirs(a.out_dir, exist_ok=True)
    head = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'mesh': f'gyroid, 4 periods, iso 1.5, {a.size}^3'}
    for what, name, fn in (('timing', 'mesh_distance.json', lambda: timing(v, f, a.size, a.samples, dev)),
                           ('cleanup', 'mesh_distance_cleanup.json', lambda: cleanup(v, f, a.size, a.samples))):
        if what in a.what:
            out = dict(head, flops_per_test=FLOPS_PER_TEST, peak_fp64_vector_tflops=PEAK_FP64_VECTOR_TFLOPS, **fn()) if what == 'timing' \
                else dict(head, **fn(), **({'scene1_sigma_against_tsdf': scene1(dev, a.iters, a.size, a.samples)} if a.scene1 else {}))
            with open(os.path.join(a.out_dir, name), 'w') as fh:
                json.dump(out, fh, indent=1)
            print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
