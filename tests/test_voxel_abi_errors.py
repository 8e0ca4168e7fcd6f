"""The argument checks of the mesh voxelisation (csrc/mesh_voxel.hip), without a GPU: every entry point returns MVIP_EINVAL (-1)
before its first device call for a NULL operand, a negative or oversized count, cells outside 1..512, a non-finite or non-positive
inv, a non-finite bmin or a bad `axes`; and the ops raise ValueError for what they can see on the host.  The pointers of the
malformed calls are never read: 64 stands for "not NULL"."""
import ctypes
import math

import pytest
import torch

from mvip_nerf_amd import _lib, ops

EINVAL = -1
P = 64               # a non-NULL device pointer that no call here reads
P0 = None


def box(*v):
    return (ctypes.c_float * 6)(*(v or (0, 0, 0, 1, 1, 1)))


def cells(*c):
    return (ctypes.c_int * 3)(*(c or (4, 4, 4)))


BAD_GRIDS = [(box(), cells(0, 4, 4)), (box(), cells(4, 513, 4)), (box(), cells(4, 4, -1)), (box(0, 0, 0, 1, 0, 1), cells()),
             (box(0, 0, 0, 1, 1, -2), cells()), (box(0, 0, 0, math.inf, 1, 1), cells()), (box(0, 0, 0, 1, math.nan, 1), cells()),
             (box(math.nan, 0, 0, 1, 1, 1), cells()), (box(0, -math.inf, 0, 1, 1, 1), cells()), (None, cells()), (box(), None)]
BAD_MESHES = [(P0, P, 3, 1), (P, P0, 3, 1), (P, P, -1, 1), (P, P, 3, -1), (P, P, 2 ** 31, 1), (P, P, 3, (2 ** 31 - 1) // 3 + 1)]


def test_surface_argument_checks():
    f = _lib.load().mvip_voxel_surface
    for b, c in BAD_GRIDS:
        assert f(P, P, 3, 1, b, c, P, P, P0) == EINVAL
    for v, fa, nv, nf in BAD_MESHES:
        assert f(v, fa, nv, nf, box(), cells(), P, P, P0) == EINVAL
    assert f(P, P, 3, 1, box(), cells(), P0, P, P0) == EINVAL
    assert f(P, P, 3, 1, box(), cells(), P, P0, P0) == EINVAL
    assert f(P0, P0, 0, 0, box(), cells(), P0, P, P0) == EINVAL          # an empty mesh still needs its outputs


def test_crossings_and_fill_argument_checks():
    lib = _lib.load()
    f = lib.mvip_voxel_crossings
    for b, c in BAD_GRIDS:
        assert f(P, P, 3, 1, b, c, 3, P, P, P0) == EINVAL
    for v, fa, nv, nf in BAD_MESHES:
        assert f(v, fa, nv, nf, box(), cells(), 3, P, P, P0) == EINVAL
    for axes in (-1, 4, 7):
        assert f(P, P, 3, 1, box(), cells(), axes, P, P, P0) == EINVAL
        assert lib.mvip_voxel_fill(P, cells(), axes, P, P, P0) == EINVAL
        assert lib.mvip_voxel_scratch_words(cells(), axes) == -1
    assert f(P, P, 3, 1, box(), cells(), 3, P0, P, P0) == EINVAL
    assert f(P, P, 3, 1, box(), cells(), 3, P, P0, P0) == EINVAL
    g = lib.mvip_voxel_fill
    for c in (None, cells(0, 1, 1), cells(1, 1, 600)):
        assert g(P, c, 3, P, P, P0) == EINVAL
        assert lib.mvip_voxel_scratch_words(c, 3) == -1
    assert g(P0, cells(), 3, P, P, P0) == EINVAL
    assert g(P, cells(), 3, P0, P, P0) == EINVAL
    assert g(P, cells(), 3, P, P0, P0) == EINVAL


def test_scratch_words():
    w = _lib.load().mvip_voxel_scratch_words
    assert w(cells(5, 3, 70), 0) == 5 * 3 * 3 and w(cells(5, 3, 70), 3) == 3 * 5 * 3 * 3
    assert w(cells(512, 512, 512), 3) == 3 * 512 * 512 * 16 and w(cells(1, 1, 1), 2) == 1 and w(cells(2, 2, 32), 1) == 4


def test_ops_refuse_what_the_host_can_see():
    v, f = torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)
    good = ([0, 0, 0, 1, 1, 1], (4, 4, 4))
    for op in (ops.mesh_voxelize_surface, ops.mesh_voxelize_solid):
        with pytest.raises(ValueError, match='GPU'):
            op(v, f, *good)                                              # CPU tensors
        with pytest.raises(ValueError, match='verts'):
            op(v.double(), f, *good)
        with pytest.raises(ValueError, match='faces'):
            op(v, f.long(), *good)
        with pytest.raises(ValueError, match='faces'):
            op(v, f.reshape(3), *good)
        with pytest.raises(ValueError, match='GPU'):
            op(v.numpy(), f, *good)
