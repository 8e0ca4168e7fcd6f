"""Connected components without a GPU: the numpy restatement (tests/components_numpy.py) against scipy.ndimage.label and on
hand-made cases, the Python argument checks that raise before any launch, the C-ABI declarations and the argument checks of
the five entry points (the style of tests/test_abi_errors.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_numpy as C                             # noqa: E402

from mvip_nerf_amd import _lib, mesh, ops                 # noqa: E402
from mvip_nerf_amd.occupancy import OccupancyGrid         # noqa: E402
from mvip_nerf_amd.region import Region                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mvip_components_pack', 'mvip_components_groups', 'mvip_components_label', 'mvip_components_rank',
           'mvip_components_select')

RANDOM_SHAPES = [(5, 7, 33), (3, 4, 31), (1, 1, 70), (9, 1, 1), (1, 1, 1)]
SNAKES = {(17, 17, 40): 3320, (9, 9, 37): 949, (5, 7, 33): 407}
# (shape, p, connectivity, components, cells of the largest)
BIG = [((64, 64, 64), 0.34, 6, 11729, 56481), ((64, 64, 64), 0.12, 26, 2348, 25110), ((40, 33, 64), 0.34, 6, 3727, 17208)]


def random_bits(shape, p=0.5):
    return np.random.RandomState(7).rand(*shape) < p


# ---- the restatement ------------------------------------------------------------------------------------------------------

def _scipy_label(bits, connectivity):
    ndi = pytest.importorskip('scipy.ndimage')
    lab, n = ndi.label(bits, ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    return lab, n


@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('shape', RANDOM_SHAPES + [(2, 2, 2), (2, 3, 5)] + list(SNAKES))
def test_restatement_equals_scipy(shape, connectivity):
    cases = [random_bits(shape)]
    if shape in SNAKES:
        cases.append(C.snake(shape))
    for bits in cases:
        lab, n = _scipy_label(bits, connectivity)
        labels, sizes, first = C.components(bits, connectivity)
        assert len(sizes) == n and np.array_equal(labels, lab)
        flat = lab.reshape(-1)
        assert np.array_equal(sizes, np.bincount(flat, minlength=n + 1)[1:])
        assert np.array_equal(first, [np.flatnonzero(flat == c)[0] for c in range(1, n + 1)])


@pytest.mark.parametrize('shape,p,connectivity,count,largest', BIG)
def test_restatement_equals_scipy_on_the_large_fields(shape, p, connectivity, count, largest):
    bits = random_bits(shape, p)
    lab, n = _scipy_label(bits, connectivity)
    labels, sizes, first = C.components(bits, connectivity)
    assert n == count and np.array_equal(labels, lab)
    assert len(sizes) == count and sizes.max() == largest


def test_hand_made_cases():
    corners = np.zeros((2, 2, 2), bool)
    corners[0, 0, 0] = corners[1, 1, 1] = True
    assert list(C.components(corners, 6)[1]) == [1, 1] and list(C.components(corners, 26)[1]) == [2]
    wrap = np.zeros((2, 3, 5), bool)                     # linear indices 4 and 5: adjacent numbers, cells apart
    wrap[0, 0, 4] = wrap[0, 1, 0] = True
    for conn in (6, 26):
        labels, sizes, first = C.components(wrap, conn)
        assert list(sizes) == [1, 1] and list(first) == [4, 5] and labels[0, 0, 4] == 1 and labels[0, 1, 0] == 2
    for shape, cells in SNAKES.items():
        s = C.snake(shape)
        assert s.sum() == cells
        for conn in (6, 26):
            assert list(C.components(s, conn)[1]) == [cells]
    assert C.components(np.zeros((3, 3, 3), bool))[1].size == 0
    assert list(C.components(np.ones((3, 4, 5), bool))[1]) == [60]


def test_pack_unpack_and_select():
    bits = random_bits((3, 4, 31))
    words = C.pack(bits)
    assert words.dtype == np.int32 and words.shape == (C.n_words(bits.size),)
    assert np.array_equal(C.unpack(words, bits.shape), bits)
    labels, sizes, first = C.components(bits, 6)
    keep = C.keep_table(sizes, first, largest=1)
    assert np.array_equal(C.unpack(C.select(labels, keep), bits.shape), labels == 1 + int(np.argmax(sizes)))
    v = np.array([np.nan, np.inf, -np.inf, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    assert list(C.unpack(C.pack_values(v, 1.0), (5,))) == [False, True, False, True, False]


def test_selection_rule_and_tie_break():
    sizes, first = np.array([3, 5, 5, 1, 5]), np.array([0, 10, 20, 30, 40])
    assert list(C.keep_table(sizes, first, largest=2)) == [0, 0, 1, 1, 0, 0]                 # ties: the lower first
    assert list(C.keep_table(sizes, first, largest=4)) == [0, 1, 1, 1, 0, 1]
    assert list(C.keep_table(sizes, first, min_cells=4)) == [0, 0, 1, 1, 0, 1]
    assert list(C.keep_table(sizes, first, largest=4, min_cells=4)) == [0, 0, 1, 1, 0, 1]    # both must hold
    assert list(C.keep_table(sizes, first, largest=1, min_cells=6)) == [0, 0, 0, 0, 0, 0]
    assert list(C.keep_table(sizes, first, containing=[4, 0])) == [0, 0, 0, 0, 1, 0]         # an alternative ...
    assert list(C.keep_table(sizes, first, largest=1, containing=[4])) == [0, 0, 1, 0, 1, 0]  # ... OR-ed in
    for kw in (dict(largest=2), dict(largest=4, min_cells=4), dict(min_cells=2), dict(largest=1, min_cells=6), dict(largest=9)):
        assert list(ops.component_keep_table(sizes, kw.get('largest'), kw.get('min_cells'))) == list(C.keep_table(sizes, first, **kw))
    assert list(ops.component_keep_table(sizes, 1, None, also=[4, 0, 77])) == [0, 0, 1, 0, 1, 0]
    assert list(ops.component_keep_table(sizes, also=[4])) == [0, 0, 0, 0, 1, 0]
    assert list(ops.component_keep_table(np.zeros(0, np.int32), 1)) == [0]


# ---- Python argument checks: before any launch -----------------------------------------------------------------------------

def _grids():
    words = torch.zeros(ops.occupancy_words((4, 4, 4)), dtype=torch.int32)
    return [cls((0, 0, 0), (1, 1, 1), (4, 4, 4), words) for cls in (OccupancyGrid, Region)]


def test_python_argument_checks():
    words = torch.zeros(2, dtype=torch.int32)
    for conn in (18, 0, None, '6'):
        with pytest.raises(ValueError, match='connectivity'):
            ops.grid_components(words, (4, 4, 4), conn)
        for g in _grids():
            with pytest.raises(ValueError, match='connectivity'):
                g.keep_components(largest=1, connectivity=conn)
        with pytest.raises(ValueError, match='connectivity'):
            mesh.remove_floaters(torch.zeros(4, 4, 4), 1.0, largest=1, connectivity=conn)
    for shape in ((4, 4, 5), (4, 4), (0, 4, 4), (769, 1, 1)):
        with pytest.raises(_lib.MvipError):
            ops.grid_components(words, shape)
    with pytest.raises(_lib.MvipError):
        ops.grid_components(torch.zeros(3, dtype=torch.int32), (4, 4, 4))
    with pytest.raises(_lib.MvipError):
        ops.grid_select(torch.zeros(8, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8))
    for g in _grids():
        with pytest.raises(ValueError, match='criterion'):
            g.keep_components()
        for kw in (dict(largest=0), dict(largest=-1), dict(largest=1.5), dict(min_cells=0), dict(largest=1, min_cells=0)):
            with pytest.raises(ValueError, match='>= 1'):
                g.keep_components(**kw)
    grid = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError, match='criterion'):
        mesh.remove_floaters(grid, 1.0)
    with pytest.raises(ValueError, match='>= 1'):
        mesh.remove_floaters(grid, 1.0, largest=0)
    with pytest.raises(ValueError, match='>= 1'):
        mesh.remove_floaters(grid, 1.0, min_points=0)
    with pytest.raises(ValueError, match='threshold'):
        mesh.remove_floaters(grid, 0.0, largest=1)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def test_header_and_binding_table_declare_the_entry_points():
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mvip_nerf.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(mvip_[a-z0-9_]+)\s*\(', txt))
    for name in SYMBOLS:
        assert name in declared and name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(_lib.load(), name)
    assert _lib.load().mvip_abi_version() == 5                   # additive change


OK, EINVAL = 0, -1
P0 = None
W = 64                                                           # a non-null address that is never dereferenced


def test_entry_point_argument_checks():
    """Before the first HIP call: a malformed call is MVIP_EINVAL, an empty call MVIP_OK, a well-formed shape with null
    operands MVIP_EINVAL.  Nothing is launched."""
    lib = _lib.load()
    # malformed: an axis of 0 or 769, connectivity 18, counts out of range, a NaN threshold
    for shape in ((0, 4, 4), (4, 769, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.mvip_components_groups(*shape) == -1
        assert lib.mvip_components_label(W, *shape, 6, W, W, W, P0) == EINVAL
        assert lib.mvip_components_rank(W, *shape, W, 1, W, W, W, P0) == EINVAL
    assert lib.mvip_components_groups(768, 768, 768) == (768 ** 3 + 1023) // 1024
    assert lib.mvip_components_groups(1, 1, 1) == 1
    for conn in (18, 0, 8, 27):
        assert lib.mvip_components_label(W, 4, 4, 4, conn, W, W, W, P0) == EINVAL
    assert lib.mvip_components_rank(W, 4, 4, 4, W, -1, W, W, W, P0) == EINVAL
    assert lib.mvip_components_rank(W, 4, 4, 4, W, 65, W, W, W, P0) == EINVAL
    assert lib.mvip_components_pack(W, -1, 1.0, W, P0) == EINVAL
    assert lib.mvip_components_pack(W, 768 ** 3 + 1, 1.0, W, P0) == EINVAL
    assert lib.mvip_components_pack(W, 64, float('nan'), W, P0) == EINVAL
    assert lib.mvip_components_select(W, -1, W, 0, W, P0) == EINVAL
    assert lib.mvip_components_select(W, 768 ** 3 + 1, W, 0, W, P0) == EINVAL
    assert lib.mvip_components_select(W, 64, W, -1, W, P0) == EINVAL
    assert lib.mvip_components_select(W, 64, W, 65, W, P0) == EINVAL
    # well-formed shape, null operands
    assert lib.mvip_components_pack(P0, 64, 1.0, P0, P0) == EINVAL
    assert lib.mvip_components_pack(W, 64, 1.0, P0, P0) == EINVAL
    for conn in (6, 26):
        assert lib.mvip_components_label(P0, 4, 4, 4, conn, P0, P0, P0, P0) == EINVAL
        for null in range(4):
            args = [W, W, W, W]
            args[null] = P0
            assert lib.mvip_components_label(args[0], 4, 4, 4, conn, args[1], args[2], args[3], P0) == EINVAL
    assert lib.mvip_components_rank(P0, 4, 4, 4, P0, 3, P0, P0, P0, P0) == EINVAL
    assert lib.mvip_components_rank(W, 4, 4, 4, W, 3, W, W, P0, P0) == EINVAL
    assert lib.mvip_components_select(P0, 64, P0, 3, P0, P0) == EINVAL
    assert lib.mvip_components_select(W, 64, P0, 3, W, P0) == EINVAL
    # empty calls
    assert lib.mvip_components_pack(P0, 0, 1.0, P0, P0) == OK
    assert lib.mvip_components_rank(P0, 4, 4, 4, P0, 0, P0, P0, P0, P0) == OK
    assert lib.mvip_components_select(P0, 0, P0, 0, P0, P0) == OK
