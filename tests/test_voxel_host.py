"""The __host__ __device__ functions of csrc/mesh_voxel.hip walked ON THE HOST by the stand-alone program
tools/voxel_host_check.hip, compiled with the host sanitizers (address, undefined), over the cases of tests/test_voxel.py,
against the numpy restatement, bit for bit.  No GPU: the arithmetic the kernels share with this program is checked before a
kernel runs; the kernels' own part (the wave path, the prefix and combine launches) is tests/test_voxel.py's."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_raycast_numpy as C                           # noqa: E402
import test_voxel as T                                   # noqa: E402
import voxel_numpy as V                                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return next((c for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc') if c and os.path.exists(c)), None)


def cases():
    for level in (2, 3):
        v, f = C.icosphere(level, 0.8)
        for cells in T.GRIDS:
            yield v, f, V.grid_box(*T.BOX1, cells), cells
    for name in T.CASES:
        yield T.CASES[name]()


@pytest.mark.skipif(_hipcc() is None, reason='needs hipcc')
def test_host_walk_of_the_shared_functions_equals_the_restatement(tmp_path):
    exe, data = str(tmp_path / 'voxel_host_check'), str(tmp_path / 'cases.bin')
    r = subprocess.run([_hipcc(), '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-Xarch_host',
                        '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        os.path.join(ROOT, 'tools', 'voxel_host_check.hip'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blobs, n = [], 0
    for v, f, box, cells in cases():
        v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
        ref = T.reference(v, f, box, cells)
        blobs += [np.asarray([len(v), len(f), *cells], np.int32), np.asarray(box, np.float32), v, f]
        for axes in V.AXES:
            words, odd, dropped = ref[axes]
            blobs += [np.asarray(words, np.int32), np.asarray(list(odd) + [dropped], np.int32)]
        blobs += [np.asarray(ref['surface'][0], np.int32), np.asarray([ref['surface'][1]], np.int32)]
        n += 1
    with open(data, 'wb') as fh:
        fh.write(np.asarray([n], np.int32).tobytes())
        for b in blobs:
            fh.write(np.ascontiguousarray(b).tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')      # (the HIP runtime's start-up allocations are not this program's)
    r = subprocess.run([exe, data], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f'{n} cases, 0 mismatches' in r.stdout
