"""numpy restatement of connected components on a bit array (csrc/components.hip, ops.grid_pack / grid_components /
grid_select, BitGrid.keep_components), written from the conventions alone -- the role tests/occupancy_numpy.py has for the
occupancy grid.

Array [nx, ny, nz], z fastest; element l = (i ny + j) nz + k is bit l & 31 of int32 word l >> 5, tail bits zero.  Two set
elements are neighbours at connectivity 6 if they differ by one step on one axis, at 26 if by at most one step on every
axis; a neighbour exists only inside the array.  Components are numbered 1, 2, ... by ascending lowest linear index;
labels is 0 on clear elements; sizes[c - 1] / first[c - 1] are the element count and the lowest linear index of component c.
"""
import collections

import numpy as np


def n_words(n):
    return (int(n) + 31) // 32


def pack(bits):
    """bool array (any shape) -> int32 words of its flattening."""
    flat = np.asarray(bits, bool).reshape(-1)
    padded = np.zeros(n_words(flat.size) * 32, np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder='little').reshape(-1).view('<u4').astype(np.uint32).view(np.int32)


def unpack(words, shape):
    """int32 words -> bool array of `shape`; asserts the unused tail bits are zero."""
    n = int(np.prod(shape))
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32).astype('<u4')
    assert w.shape == (n_words(n),)
    bits = np.unpackbits(w.view(np.uint8), bitorder='little')
    assert not bits[n:].any(), 'tail bits must be zero'
    return bits[:n].astype(bool).reshape(shape)


def pack_values(values, threshold):
    """bit l = values[l] >= threshold in fp32 (NaN: clear)."""
    with np.errstate(invalid='ignore'):
        return pack(np.asarray(values, np.float32) >= np.float32(threshold))


def offsets(connectivity):
    assert connectivity in (6, 26)
    out = []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for dk in (-1, 0, 1):
                steps = abs(di) + abs(dj) + abs(dk)
                if steps and (connectivity == 26 or steps == 1):
                    out.append((di, dj, dk))
    return out


def components(bits, connectivity=6):
    """(labels int32 [nx, ny, nz], sizes int32 [n], first int32 [n]) by breadth-first search from each unlabelled set
    element in ascending linear order: the search that starts at l finds the component whose lowest index is l."""
    bits = np.asarray(bits, bool)
    nx, ny, nz = bits.shape
    labels = np.zeros(bits.shape, np.int32)
    sizes, first = [], []
    offs = offsets(connectivity)
    for l in np.flatnonzero(bits.reshape(-1)):
        i, r = divmod(int(l), ny * nz)
        j, k = divmod(r, nz)
        if labels[i, j, k]:
            continue
        c = len(sizes) + 1
        labels[i, j, k] = c
        count = 0
        queue = collections.deque([(i, j, k)])
        while queue:
            a, b, d = queue.popleft()
            count += 1
            for di, dj, dk in offs:
                x, y, z = a + di, b + dj, d + dk
                if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and bits[x, y, z] and not labels[x, y, z]:
                    labels[x, y, z] = c
                    queue.append((x, y, z))
        sizes.append(count)
        first.append(int(l))
    return labels, np.asarray(sizes, np.int32), np.asarray(first, np.int32)


def keep_table(sizes, first, largest=None, min_cells=None, containing=None):
    """uint8 [n + 1], keep[0] = 0.  largest = k: the k components with the most elements, ties to the lower `first`;
    min_cells = m: at least m elements; a component must meet each of the two that is given.  containing: labels kept in
    addition (0 = none).  With neither largest nor min_cells only `containing` is kept."""
    n = len(sizes)
    keep = np.zeros(n + 1, np.uint8)
    if largest is not None or min_cells is not None:
        chosen = set(range(n))
        if largest is not None:
            ranked = sorted(range(n), key=lambda c: (-int(sizes[c]), int(first[c])))
            chosen &= set(ranked[:largest])
        if min_cells is not None:
            chosen &= {c for c in range(n) if sizes[c] >= min_cells}
        for c in chosen:
            keep[c + 1] = 1
    for lab in ([] if containing is None else containing):
        if lab > 0:
            keep[int(lab)] = 1
    return keep


def select(labels, keep):
    """int32 words of the elements whose component is kept."""
    return pack(np.asarray(keep, bool)[np.asarray(labels)])


def snake(shape):
    """One long component (see tests/test_components.py): in planes i = 0, 2, 4, ... the full z rows at j = 0, 2, 4, ...,
    visited boustrophedon (the j order reverses in every second plane), consecutive rows joined by one cell at the
    alternating z end -- the cell between them in j, or the cell at i + 1 where the plane changes."""
    nx, ny, nz = shape
    bits = np.zeros(shape, bool)
    rows = []
    for p, i in enumerate(range(0, nx, 2)):
        js = list(range(0, ny, 2))
        rows += [(i, j) for j in (js[::-1] if p % 2 else js)]
    for r, (i, j) in enumerate(rows):
        bits[i, j, :] = True
        if r + 1 < len(rows):
            i2, j2 = rows[r + 1]
            end = nz - 1 if r % 2 == 0 else 0
            if i2 == i:
                bits[i, (j + j2) // 2, end] = True
            else:
                bits[i + 1, j, end] = True
    return bits
