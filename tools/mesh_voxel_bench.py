"""Mesh voxelisation timings (profiles/mesh_voxel.json): csrc/mesh_voxel.hip on the marching-cubes mesh of the 4-period gyroid at
256^3 (2.5 M triangles, the mesh of tools/mesh_topology_bench.py) and on its clustering at 8 lattice steps (large triangles:
the wave path), at 128^3, 256^3 and 512^3 cells of the box [-1, 1]^3: the surface entry point, the crossings entry point per
axis and for the three together, the fill (prefix parity of three grids, majority, the output words), each on preallocated
buffers, and the whole ops calls with their allocations and the one read-back.  HIP-event times, the median of 5 windows after a
warm-up.  Beside them: ops.mesh_face_grid of the same mesh (the yardstick of the other mesh structures), the bytes per second
the fill achieves against a device copy of as many bytes, and the share of the lanes that have a cell / a sample in the wave
path's iterations -- COMPUTED from the faces' ranges in fp64 with torch (the ranges the kernels form), not counted by the
kernels.  A record, not a gate.

  python tools/mesh_voxel_bench.py [--out profile_out/mesh_voxel.json] [--size 256] [--cells 128 256 512] [--commit HASH]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mvip_nerf_amd import _lib, bitgrid, mesh, ops                   # noqa: E402
from mvip_nerf_amd._lib import ptr, stream, call                     # noqa: E402
from tools.mesh_bench import event_ms, gyroid                        # noqa: E402

I32 = torch.int32
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def lane_utilisation(v, f, box, cells):
    """(surface, crossings per axis): over the faces the wave walks, useful lane-iterations / (64 x iterations); None: no such face"""
    b = torch.tensor(box, dtype=torch.float32, device=v.device).double()
    g = (v.double() - b[:3]) * b[3:]
    G = g[f.long()]                                                   # [F, 3, 3]
    c = torch.tensor(cells, device=v.device, dtype=torch.float64)
    m = 2.0 ** -12
    lo = torch.clamp(torch.floor(G.min(1).values - m), min=0.0)
    hi = torch.minimum(torch.floor(G.max(1).values + m), c - 1.0)
    n = torch.clamp(hi - lo + 1.0, min=0.0).prod(1)
    big = n > 64
    surf = float(n[big].sum() / (64.0 * torch.ceil(n[big] / 64.0).sum())) if bool(big.any()) else None
    out = []
    for a in range(3):
        bb, cc = (a + 1) % 3, (a + 2) % 3
        X, Y = torch.round(256.0 * G[:, :, bb]), torch.round(256.0 * G[:, :, cc])
        x0 = torch.clamp(torch.floor((X.min(1).values + 127.0) / 256.0), min=0.0)
        x1 = torch.clamp(torch.floor((X.max(1).values - 128.0) / 256.0), max=cells[bb] - 1.0)
        y0 = torch.clamp(torch.floor((Y.min(1).values + 127.0) / 256.0), min=0.0)
        y1 = torch.clamp(torch.floor((Y.max(1).values - 128.0) / 256.0), max=cells[cc] - 1.0)
        w, h = torch.clamp(x1 - x0 + 1.0, min=0.0), torch.clamp(y1 - y0 + 1.0, min=0.0)
        big = w * h > 16
        out.append(float((w * h)[big].sum() / (64.0 * (torch.ceil(w[big] / 8.0) * torch.ceil(h[big] / 8.0)).sum())) if bool(big.any()) else None)
    return surf, out, int((n > 64).sum())


def row(m, n_cells):
    v, f = m.verts, m.faces
    Nv, F, dev = int(v.shape[0]), int(f.shape[0]), v.device
    cells = (n_cells,) * 3
    grid = bitgrid.BitGrid(LO, HI, cells, torch.zeros(ops.occupancy_words(cells), device=dev, dtype=I32))
    box = grid.box()
    cbox, ccells = (ctypes.c_float * 6)(*box), (ctypes.c_int * 3)(*cells)
    words, counters = torch.empty_like(grid.words), torch.empty(ops.VOXEL_COUNTERS, device=dev, dtype=I32)
    n_scratch = _lib.load().mvip_voxel_scratch_words(ccells, 3)
    scratch = torch.empty(n_scratch, device=dev, dtype=I32)
    ms = lambda fn: round(event_ms(fn, warmup=1, reps=5)[0], 4)
    mesh_args = (ptr(v), ptr(f, I32), Nv, F, cbox, ccells)
    out = {'cells': list(cells), 'ms_surface': ms(lambda: call('mvip_voxel_surface', *mesh_args, ptr(words, I32), ptr(counters, I32), stream()))}
    for a, name in enumerate(ops.VOXEL_AXES):
        out['ms_crossings_' + name] = ms(lambda: call('mvip_voxel_crossings', *mesh_args, a, ptr(scratch, I32), ptr(counters, I32), stream()))
    out['ms_fill_majority'] = ms(lambda: call('mvip_voxel_fill', ptr(scratch, I32), ccells, 3, ptr(words, I32), ptr(counters, I32), stream()))
    # the fill reads and writes each of the three crossing grids once (prefix), reads them again (combine) and writes the words
    fill_bytes = 4 * (3 * n_scratch + int(words.shape[0]))
    src = torch.empty(fill_bytes // 8, device=dev, dtype=I32)
    dst = torch.empty_like(src)
    ms_copy = ms(lambda: dst.copy_(src))
    out.update(fill_bytes=fill_bytes, fill_gb_per_s=round(fill_bytes / out['ms_fill_majority'] / 1e6, 1), ms_copy_same_bytes=ms_copy,
               copy_gb_per_s=round(fill_bytes / ms_copy / 1e6, 1))
    out['ms_api_mesh_voxelize_surface'] = ms(lambda: ops.mesh_voxelize_surface(v, f, box, cells))
    out['ms_api_mesh_voxelize_solid_majority'] = ms(lambda: ops.mesh_voxelize_solid(v, f, box, cells))
    out['ms_api_mesh_voxelize_solid_z'] = ms(lambda: ops.mesh_voxelize_solid(v, f, box, cells, 'z'))
    _, odd, dropped = ops.mesh_voxelize_solid(v, f, box, cells)
    g, rep = mesh.voxelize(m, LO, HI, cells)
    surf, cross, n_wave = lane_utilisation(v, f, box, cells)
    out.update(odd_columns=odd, dropped=dropped, set_cells_both=rep['count'], volume_both=rep['volume'], faces_on_the_surface_wave_path=n_wave,
               lane_utilisation_surface_wave_path=surf, lane_utilisation_crossings_wave_path=cross)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--cells', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--commit', default='')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    a.out = a.out or os.path.join(ROOT, 'profile_out', 'mesh_voxel.json')
    n = a.size
    v, f, normals = mesh.marching_cubes(gyroid(n, dev), 1.5, LO, HI)
    m = mesh.Mesh(v, f, normals, None)
    coarse = mesh.simplify(m, 8.0 * 2.0 / (n - 1))
    ms = lambda fn: round(event_ms(fn, warmup=1, reps=5)[0], 4)
    out = {'commit': a.commit, 'device': torch.cuda.get_device_name(0), 'mesh': 'gyroid, 4 periods, iso 1.5', 'grid': [n, n, n], 'meshes': []}
    for name, mm in (('marching cubes', m), ('clustered at 8 lattice steps', coarse)):
        rec = {'mesh': name, 'vertices': int(mm.verts.shape[0]), 'triangles': int(mm.faces.shape[0]),
               'ms_api_mesh_face_grid': ms(lambda: ops.mesh_face_grid(mm.verts, mm.faces)), 'grids': [row(mm, c) for c in a.cells]}
        out['meshes'].append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
