"""Topology report of a triangle mesh (mesh.topology, csrc/mesh_topology.hip): components, boundary / non-manifold /
inconsistently oriented edges, Euler characteristic and genus per component, boundary loops.  The mesh is a PLY file as
mesh.save_ply writes it (tools/extract_mesh.py).  Prints the report as one JSON line.

  python tools/mesh_topology.py A.ply [--connectivity edge|vertex] [--components N]

--components N: the per-component rows printed (the first N in label order = by lowest face; default 16).  The totals and the
number of components always cover the whole mesh.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import mesh                                                 # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('a')
    ap.add_argument('--connectivity', choices=('edge', 'vertex'), default='edge')
    ap.add_argument('--components', type=int, default=16, metavar='N', help='per-component rows printed')
    a = ap.parse_args(argv)
    if a.components < 0:
        ap.error('--components must be >= 0')
    rep = mesh.topology(mesh.load_ply(a.a, device=torch.device('cuda', 0)), a.connectivity)
    rep['per_component'] = rep['per_component'][:a.components]
    print(json.dumps(rep))
    return 0


if __name__ == '__main__':
    sys.exit(main())
