"""Distance report of two triangle meshes (evaluate.mesh_distance_metrics, csrc/mesh_distance.hip): Chamfer and sampled Hausdorff
distance, mean / RMS / maximum per direction, precision / recall / F-score at the tolerances --tau, normal consistency.  The
meshes are PLY files as mesh.save_ply writes them (tools/extract_mesh.py).  Prints the report as one JSON line.

  python tools/mesh_distance.py A.ply B.ply [--samples K] [--tau T ...]

--samples K: K^2 equal-area sample points per face (default 2).  Precision is the share of A's area within tau of B, recall the
share of B's area within tau of A.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import evaluate, mesh                                       # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--samples', type=int, default=2, metavar='K', help='K^2 sample points per face')
    ap.add_argument('--tau', type=float, nargs='*', default=[], help='tolerances of precision / recall / F-score')
    a = ap.parse_args(argv)
    if a.samples < 1:
        ap.error('--samples must be >= 1')
    dev = torch.device('cuda', 0)
    rep = evaluate.mesh_distance_metrics(mesh.load_ply(a.a, device=dev), mesh.load_ply(a.b, device=dev), samples=a.samples,
                                         thresholds=a.tau)
    print(json.dumps(rep))
    return 0


if __name__ == '__main__':
    sys.exit(main())
