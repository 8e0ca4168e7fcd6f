"""The __host__ __device__ functions of csrc/mesh_distance_device.h and csrc/mesh_sdf.hip -- point_triangle with its feature
code, the pseudonormal of the closest feature, the sign -- walked ON THE HOST by the stand-alone program
tools/mesh_sdf_host_check.hip, compiled with the host sanitizers (address, undefined), against the numpy restatement, bit for
bit.  No GPU: the arithmetic the kernels share with this program is checked before a kernel runs; the kernels' own part (the
walk over the face grid, the band, the lattice) is tests/test_mesh_sdf.py's."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_distance_numpy as D                          # noqa: E402
import mesh_sdf_numpy as S                               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return next((c for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc') if c and os.path.exists(c)), None)


def cases():
    for build in (S.tetrahedron, S.spike, S.fan_spike, lambda: D.cube_mesh(0.5), S.open_degenerate):
        v, f = build()
        yield v, f, S.query_set(v, f, 300, 3)


@pytest.mark.skipif(_hipcc() is None, reason='needs hipcc')
def test_host_walk_of_the_shared_functions_equals_the_restatement(tmp_path):
    exe, data = str(tmp_path / 'mesh_sdf_host_check'), str(tmp_path / 'cases.bin')
    r = subprocess.run([_hipcc(), '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Xarch_host',
                        '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        os.path.join(ROOT, 'tools', 'mesh_sdf_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blobs, n, queries, feats = [], 0, 0, set()
    for v, f, pts in cases():
        P, twin = S.vertex_pseudonormals(v, f), S.twins(f, len(v))
        sd, face, point, feat, _ = S.signed_distance(pts, v, f, P=P, twin=twin)
        blobs += [np.asarray([len(v), len(f), len(pts)], np.int32), v.astype(np.float32), f.astype(np.int32), twin.astype(np.int32),
                  P.astype(np.float64), pts, face.astype(np.int32), feat.astype(np.int32), sd.astype(np.float32), point.astype(np.float32)]
        n += 1
        queries += len(pts)
        feats |= set(np.unique(feat).tolist())
    assert feats == {-1, 0, 1, 2, 3, 4, 5, 6}
    with open(data, 'wb') as fh:
        fh.write(np.asarray([n], np.int32).tobytes())
        for b in blobs:
            fh.write(np.ascontiguousarray(b).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')      # (the HIP runtime's start-up allocations are not this program's)
    r = subprocess.run([exe, data], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f'{n} cases, {queries} queries, 0 mismatches' in r.stdout
