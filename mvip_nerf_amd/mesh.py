"""Triangle-mesh export of a trained radiance field (beyond the reference: MVIP-NeRF only renders depth / normal images).

density_grid() samples sigma on a dense grid with the model's own no-grad query path (`render_kwargs['network_query_fn']`:
the fused 8x256 MLP kernel for create_nerf, the fused hash-grid kernel for create_nerf_tcnn); marching_cubes() turns it into
an indexed, crack-free triangle mesh with the HIP passes of csrc/mcubes.hip; extract_mesh() does both and colours the
vertices; save_ply() writes the result.  fuse_depths() / extract_mesh_tsdf() mesh what the renderer sees instead: the
rendered depth maps of the views fused into a truncated signed distance field (csrc/tsdf.hip), zero level set.  There is no CPU path: grids and meshes live on the device until save_ply.
smooth() / simplify() / vertex_normals() clean the raw marching-cubes output up (csrc/mesh_ops.hip): Taubin smoothing
against the lattice staircase, vertex clustering to a tenth of the triangles, and normals from the faces alone for a mesh
that no longer sits on its lattice.
render_views() / visible_faces() / keep_faces() look at a mesh through the cameras again (csrc/raster.hip): the disparity,
face-id and colour maps it presents to each view, the faces any view sees, and the mesh of those alone.
bake_texture() / colors_from_views() / render_textured() / save_obj() take the colour from the views instead of the field
(csrc/texture.hip): a per-face texture atlas or vertex colours blended from the images of the cameras that see each point,
the textured mesh rendered back into a camera, and OBJ + MTL + PNG export.
load_ply() reads back what save_ply() wrote, bit for bit; how far two meshes lie apart is evaluate.mesh_distance_metrics
(csrc/mesh_distance.hip).
cast_rays() / cast_views() / face_openness() / drop_interior() ask what a ray hits (csrc/mesh_raycast.hip): the first face along
render_rays' own ray rows, frames without the rasteriser's near-plane drop, and the faces of interior shells that see nothing
but mesh.
signed_distance() / sdf_grid() / remesh() say on which side of the surface a point lies and how far (csrc/mesh_sdf.hip), on
points or on a lattice, and extract the mesh again from that field: closed and evenly tessellated, optionally offset;
margin_cells() is the metric margin of Region.from_mesh / OccupancyGrid.from_mesh.

Conventions (shared with csrc/mcubes.hip and the test restatement tests/mc_numpy.py): grid [nx, ny, nz], z fastest; point
(i, j, k) sits at bmin + (i, j, k) * (bmax - bmin) / (n - 1), in fp32 arithmetic; a corner is inside iff sigma >= threshold
(threshold > 0); t = (threshold - v0) / (v1 - v0), p = p0 + t (p1 - p0); vertices are ordered by (point, axis), triangles
by (cell, table slot); faces are counter-clockwise seen from outside (decreasing sigma), so a closed surface has positive
signed volume.  Normals are -grad sigma (central differences), normalised.
"""
import collections
import math
import os

import numpy as np
import torch

from . import ops

# Corner c of a cell = (dx, dy, dz) with c = dx + 2 dy + 4 dz; bit c of the cube index is set iff corner c is inside.
# Edge e = 4 * axis + r runs from the corner with the two other offsets (r & 1, r >> 1), in axis order, along `axis`.
# Row `cube` lists up to five triangles as edge triples, -1 terminated.  The table was derived, not transcribed: on every
# cell face the crossing edges are paired so that each inside corner of an ambiguous face (two inside corners on a
# diagonal) is cut off on its own; that choice depends on the face's four corners alone, so the two cells sharing a face
# cut it the same way and the surface has no cracks.  The face segments chain into closed loops; each loop is triangulated
# (a fan where one qualifies) with no diagonal between two edges of one cell face, since the neighbour across that face
# could draw the same diagonal and the mesh edge would then have four triangles.  Every triangle is wound
# counter-clockwise seen from the outside corners.
# tests/test_mesh_cpu.py checks closedness, orientation and every ambiguous configuration on this table.
TRI_TABLE = (
    (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 8, 1, 8, 9, 1, 9, 5, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 9, 1, 9, 11, -1, -1, -1, -1, -1, -1, -1),
    (4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 10, 0, 10, 8, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 10, 0, 10, 4, -1, -1, -1, -1, -1, -1, -1),
    (8, 9, 11, 8, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 9, 5, 2, 5, 4, 2, 4, 6, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 10, 4, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 6, 1, 6, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1, -1),
    (1, 5, 11, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 2, 1, 5, 11, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 1, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 6, 1, 6, 2, 1, 2, 9, 1, 9, 11, -1, -1, -1, -1),
    (2, 8, 6, 4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 10, 0, 10, 6, 0, 6, 2, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 10, 0, 10, 4, 2, 8, 6, -1, -1, -1, -1),
    (2, 9, 11, 2, 11, 10, 2, 10, 6, -1, -1, -1, -1, -1, -1, -1),
    (2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 7, 5, 2, 5, 4, 2, 4, 8, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 8, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 5, 1, 10, 4, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 8, 1, 8, 2, 1, 2, 7, 1, 7, 5, -1, -1, -1, -1),
    (1, 5, 11, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 11, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 11, 0, 11, 1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 2, 1, 2, 7, 1, 7, 11, -1, -1, -1, -1),
    (2, 7, 9, 4, 5, 11, 4, 11, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 10, 0, 10, 8, 2, 7, 9, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 11, 0, 11, 10, 0, 10, 4, -1, -1, -1, -1),
    (2, 7, 11, 2, 11, 10, 2, 10, 8, -1, -1, -1, -1, -1, -1, -1),
    (6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 7, 0, 7, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 8, 6, 0, 6, 7, 0, 7, 5, -1, -1, -1, -1, -1, -1, -1),
    (4, 6, 7, 4, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, 6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 9, -1, -1, -1, -1),
    (0, 8, 6, 0, 6, 7, 0, 7, 5, 1, 10, 4, -1, -1, -1, -1),
    (1, 10, 6, 1, 6, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 11, 6, 7, 9, 6, 9, 8, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 7, 0, 7, 9, 1, 5, 11, -1, -1, -1, -1),
    (0, 8, 6, 0, 6, 7, 0, 7, 11, 0, 11, 1, -1, -1, -1, -1),
    (1, 4, 6, 1, 6, 7, 1, 7, 11, -1, -1, -1, -1, -1, -1, -1),
    (4, 5, 11, 4, 11, 10, 6, 7, 9, 6, 9, 8, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 10, 0, 10, 6, 0, 6, 7, 0, 7, 9, -1),
    (0, 8, 6, 0, 6, 7, 0, 7, 11, 0, 11, 10, 0, 10, 4, -1),
    (6, 7, 11, 6, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 6, 10, 4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1),
    (1, 3, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 3, 0, 3, 6, 0, 6, 8, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 3, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1, -1),
    (1, 3, 6, 1, 6, 8, 1, 8, 9, 1, 9, 5, -1, -1, -1, -1),
    (1, 5, 11, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 11, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 1, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 9, 1, 9, 11, 3, 6, 10, -1, -1, -1, -1),
    (3, 6, 4, 3, 4, 5, 3, 5, 11, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 3, 0, 3, 6, 0, 6, 8, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 3, 0, 3, 6, 0, 6, 4, -1, -1, -1, -1),
    (3, 6, 8, 3, 8, 9, 3, 9, 11, -1, -1, -1, -1, -1, -1, -1),
    (2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1, -1),
    (2, 9, 5, 2, 5, 4, 2, 4, 10, 2, 10, 3, -1, -1, -1, -1),
    (1, 3, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 3, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1, -1),
    (1, 3, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 11, 2, 8, 10, 2, 10, 3, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 3, 0, 3, 2, 1, 5, 11, -1, -1, -1, -1),
    (0, 9, 11, 0, 11, 1, 2, 8, 10, 2, 10, 3, -1, -1, -1, -1),
    (4, 10, 3, 4, 3, 2, 4, 2, 9, 4, 9, 11, 4, 11, 1, -1),
    (2, 8, 4, 2, 4, 5, 2, 5, 11, 2, 11, 3, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 3, 0, 3, 2, -1, -1, -1, -1, -1, -1, -1),
    (11, 3, 2, 11, 2, 8, 11, 8, 4, 11, 4, 0, 11, 0, 9, -1),
    (2, 9, 11, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 5, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (2, 7, 5, 2, 5, 4, 2, 4, 8, 3, 6, 10, -1, -1, -1, -1),
    (1, 3, 6, 1, 6, 4, 2, 7, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 3, 0, 3, 6, 0, 6, 8, 2, 7, 9, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 5, 1, 3, 6, 1, 6, 4, -1, -1, -1, -1),
    (1, 3, 6, 1, 6, 8, 1, 8, 2, 1, 2, 7, 1, 7, 5, -1),
    (1, 5, 11, 2, 7, 9, 3, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 11, 2, 7, 9, 3, 6, 10, -1, -1, -1, -1),
    (0, 2, 7, 0, 7, 11, 0, 11, 1, 3, 6, 10, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 2, 1, 2, 7, 1, 7, 11, 3, 6, 10, -1),
    (2, 7, 9, 3, 6, 4, 3, 4, 5, 3, 5, 11, -1, -1, -1, -1),
    (0, 5, 11, 0, 11, 3, 0, 3, 6, 0, 6, 8, 2, 7, 9, -1),
    (0, 2, 7, 0, 7, 11, 0, 11, 3, 0, 3, 6, 0, 6, 4, -1),
    (11, 3, 6, 11, 6, 8, 11, 8, 2, 11, 2, 7, -1, -1, -1, -1),
    (3, 7, 9, 3, 9, 8, 3, 8, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1, -1),
    (0, 8, 10, 0, 10, 3, 0, 3, 7, 0, 7, 5, -1, -1, -1, -1),
    (3, 7, 5, 3, 5, 4, 3, 4, 10, -1, -1, -1, -1, -1, -1, -1),
    (1, 3, 7, 1, 7, 9, 1, 9, 8, 1, 8, 4, -1, -1, -1, -1),
    (0, 1, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1, -1, -1, -1, -1),
    (8, 4, 1, 8, 1, 3, 8, 3, 7, 8, 7, 5, 8, 5, 0, -1),
    (1, 3, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 11, 3, 7, 9, 3, 9, 8, 3, 8, 10, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 3, 0, 3, 7, 0, 7, 9, 1, 5, 11, -1),
    (0, 8, 10, 0, 10, 3, 0, 3, 7, 0, 7, 11, 0, 11, 1, -1),
    (4, 10, 3, 4, 3, 7, 4, 7, 11, 4, 11, 1, -1, -1, -1, -1),
    (3, 7, 9, 3, 9, 8, 3, 8, 4, 3, 4, 5, 3, 5, 11, -1),
    (0, 5, 11, 0, 11, 3, 0, 3, 7, 0, 7, 9, -1, -1, -1, -1),
    (0, 8, 4, 3, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 11, 7, 4, 8, 9, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 8, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 10, 4, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 8, 1, 8, 9, 1, 9, 5, 3, 11, 7, -1, -1, -1, -1),
    (1, 5, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 7, 0, 7, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 9, 1, 9, 7, 1, 7, 3, -1, -1, -1, -1),
    (3, 10, 4, 3, 4, 5, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 7, 0, 7, 3, 0, 3, 10, 0, 10, 8, -1, -1, -1, -1),
    (0, 9, 7, 0, 7, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1, -1),
    (3, 10, 8, 3, 8, 9, 3, 9, 7, -1, -1, -1, -1, -1, -1, -1),
    (2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 2, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (2, 9, 5, 2, 5, 4, 2, 4, 6, 3, 11, 7, -1, -1, -1, -1),
    (1, 10, 4, 2, 8, 6, 3, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 6, 0, 6, 2, 3, 11, 7, -1, -1, -1, -1),
    (0, 9, 5, 1, 10, 4, 2, 8, 6, 3, 11, 7, -1, -1, -1, -1),
    (1, 10, 6, 1, 6, 2, 1, 2, 9, 1, 9, 5, 3, 11, 7, -1),
    (1, 5, 7, 1, 7, 3, 2, 8, 6, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 2, 1, 5, 7, 1, 7, 3, -1, -1, -1, -1),
    (0, 9, 7, 0, 7, 3, 0, 3, 1, 2, 8, 6, -1, -1, -1, -1),
    (1, 4, 6, 1, 6, 2, 1, 2, 9, 1, 9, 7, 1, 7, 3, -1),
    (2, 8, 6, 3, 10, 4, 3, 4, 5, 3, 5, 7, -1, -1, -1, -1),
    (0, 5, 7, 0, 7, 3, 0, 3, 10, 0, 10, 6, 0, 6, 2, -1),
    (0, 9, 7, 0, 7, 3, 0, 3, 10, 0, 10, 4, 2, 8, 6, -1),
    (9, 7, 3, 9, 3, 10, 9, 10, 6, 9, 6, 2, -1, -1, -1, -1),
    (2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 2, 3, 0, 3, 11, 0, 11, 5, -1, -1, -1, -1, -1, -1, -1),
    (2, 3, 11, 2, 11, 5, 2, 5, 4, 2, 4, 8, -1, -1, -1, -1),
    (1, 10, 4, 2, 3, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 8, 2, 3, 11, 2, 11, 9, -1, -1, -1, -1),
    (0, 2, 3, 0, 3, 11, 0, 11, 5, 1, 10, 4, -1, -1, -1, -1),
    (8, 2, 3, 8, 3, 11, 8, 11, 5, 8, 5, 1, 8, 1, 10, -1),
    (1, 5, 9, 1, 9, 2, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 9, 1, 9, 2, 1, 2, 3, -1, -1, -1, -1),
    (0, 2, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 2, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1),
    (2, 3, 10, 2, 10, 4, 2, 4, 5, 2, 5, 9, -1, -1, -1, -1),
    (5, 9, 2, 5, 2, 3, 5, 3, 10, 5, 10, 8, 5, 8, 0, -1),
    (0, 2, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1, -1, -1, -1, -1),
    (2, 3, 10, 2, 10, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 11, 9, 3, 9, 8, 3, 8, 6, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 6, 0, 6, 3, 0, 3, 11, 0, 11, 9, -1, -1, -1, -1),
    (0, 8, 6, 0, 6, 3, 0, 3, 11, 0, 11, 5, -1, -1, -1, -1),
    (3, 11, 5, 3, 5, 4, 3, 4, 6, -1, -1, -1, -1, -1, -1, -1),
    (1, 10, 4, 3, 11, 9, 3, 9, 8, 3, 8, 6, -1, -1, -1, -1),
    (0, 1, 10, 0, 10, 6, 0, 6, 3, 0, 3, 11, 0, 11, 9, -1),
    (0, 8, 6, 0, 6, 3, 0, 3, 11, 0, 11, 5, 1, 10, 4, -1),
    (6, 3, 11, 6, 11, 5, 6, 5, 1, 6, 1, 10, -1, -1, -1, -1),
    (1, 5, 9, 1, 9, 8, 1, 8, 6, 1, 6, 3, -1, -1, -1, -1),
    (6, 3, 1, 6, 1, 5, 6, 5, 9, 6, 9, 0, 6, 0, 4, -1),
    (0, 8, 6, 0, 6, 3, 0, 3, 1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 6, 1, 6, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (3, 10, 4, 3, 4, 5, 3, 5, 9, 3, 9, 8, 3, 8, 6, -1),
    (0, 5, 9, 3, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 8, 6, 0, 6, 3, 0, 3, 10, 0, 10, 4, -1, -1, -1, -1),
    (3, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 6, 10, 11, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (4, 8, 9, 4, 9, 5, 6, 10, 11, 6, 11, 7, -1, -1, -1, -1),
    (1, 11, 7, 1, 7, 6, 1, 6, 4, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 11, 0, 11, 7, 0, 7, 6, 0, 6, 8, -1, -1, -1, -1),
    (0, 9, 5, 1, 11, 7, 1, 7, 6, 1, 6, 4, -1, -1, -1, -1),
    (1, 11, 7, 1, 7, 6, 1, 6, 8, 1, 8, 9, 1, 9, 5, -1),
    (1, 5, 7, 1, 7, 6, 1, 6, 10, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 7, 1, 7, 6, 1, 6, 10, -1, -1, -1, -1),
    (0, 9, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 9, 1, 9, 7, 1, 7, 6, 1, 6, 10, -1),
    (4, 5, 7, 4, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 7, 0, 7, 6, 0, 6, 8, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 7, 0, 7, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1),
    (6, 8, 9, 6, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 8, 10, 2, 10, 11, 2, 11, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 11, 0, 11, 7, 0, 7, 2, -1, -1, -1, -1),
    (0, 9, 5, 2, 8, 10, 2, 10, 11, 2, 11, 7, -1, -1, -1, -1),
    (2, 9, 5, 2, 5, 4, 2, 4, 10, 2, 10, 11, 2, 11, 7, -1),
    (1, 11, 7, 1, 7, 2, 1, 2, 8, 1, 8, 4, -1, -1, -1, -1),
    (0, 1, 11, 0, 11, 7, 0, 7, 2, -1, -1, -1, -1, -1, -1, -1),
    (0, 9, 5, 1, 11, 7, 1, 7, 2, 1, 2, 8, 1, 8, 4, -1),
    (1, 11, 7, 1, 7, 2, 1, 2, 9, 1, 9, 5, -1, -1, -1, -1),
    (1, 5, 7, 1, 7, 2, 1, 2, 8, 1, 8, 10, -1, -1, -1, -1),
    (10, 1, 5, 10, 5, 7, 10, 7, 2, 10, 2, 0, 10, 0, 4, -1),
    (7, 2, 8, 7, 8, 10, 7, 10, 1, 7, 1, 0, 7, 0, 9, -1),
    (1, 4, 10, 2, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 8, 4, 2, 4, 5, 2, 5, 7, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 7, 0, 7, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (7, 2, 8, 7, 8, 4, 7, 4, 0, 7, 0, 9, -1, -1, -1, -1),
    (2, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 6, 10, 2, 10, 11, 2, 11, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 8, 2, 6, 10, 2, 10, 11, 2, 11, 9, -1, -1, -1, -1),
    (0, 2, 6, 0, 6, 10, 0, 10, 11, 0, 11, 5, -1, -1, -1, -1),
    (2, 6, 10, 2, 10, 11, 2, 11, 5, 2, 5, 4, 2, 4, 8, -1),
    (1, 11, 9, 1, 9, 2, 1, 2, 6, 1, 6, 4, -1, -1, -1, -1),
    (1, 11, 9, 1, 9, 2, 1, 2, 6, 1, 6, 8, 1, 8, 0, -1),
    (2, 6, 4, 2, 4, 1, 2, 1, 11, 2, 11, 5, 2, 5, 0, -1),
    (1, 11, 5, 2, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 9, 1, 9, 2, 1, 2, 6, 1, 6, 10, -1, -1, -1, -1),
    (0, 4, 8, 1, 5, 9, 1, 9, 2, 1, 2, 6, 1, 6, 10, -1),
    (0, 2, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 8, 1, 8, 2, 1, 2, 6, 1, 6, 10, -1, -1, -1, -1),
    (2, 6, 4, 2, 4, 5, 2, 5, 9, -1, -1, -1, -1, -1, -1, -1),
    (5, 9, 2, 5, 2, 6, 5, 6, 8, 5, 8, 0, -1, -1, -1, -1),
    (0, 2, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (8, 10, 11, 8, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 4, 10, 0, 10, 11, 0, 11, 9, -1, -1, -1, -1, -1, -1, -1),
    (0, 8, 10, 0, 10, 11, 0, 11, 5, -1, -1, -1, -1, -1, -1, -1),
    (4, 10, 11, 4, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 11, 9, 1, 9, 8, 1, 8, 4, -1, -1, -1, -1, -1, -1, -1),
    (0, 1, 11, 0, 11, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (8, 4, 1, 8, 1, 11, 8, 11, 5, 8, 5, 0, -1, -1, -1, -1),
    (1, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 5, 9, 1, 9, 8, 1, 8, 10, -1, -1, -1, -1, -1, -1, -1),
    (10, 1, 5, 10, 5, 9, 10, 9, 0, 10, 0, 4, -1, -1, -1, -1),
    (0, 8, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (1, 4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (4, 5, 9, 4, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (0, 8, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
)
assert len(TRI_TABLE) == 256 and all(len(r) == 16 for r in TRI_TABLE)

MAX_POINTS_PER_AXIS = 768

Mesh = collections.namedtuple('Mesh', ['verts', 'faces', 'normals', 'colors'])

_device_tables = {}


def device_table(device):
    """TRI_TABLE as a [256, 16] int8 tensor on `device`, uploaded once per device."""
    device = torch.device(device)
    key = (device.type, device.index)
    if key not in _device_tables:
        _device_tables[key] = torch.tensor(TRI_TABLE, dtype=torch.int8, device=device).contiguous()
    return _device_tables[key]


def _bounds(bound_min, bound_max):
    lo = np.asarray([float(v) for v in bound_min], dtype=np.float32)
    hi = np.asarray([float(v) for v in bound_max], dtype=np.float32)
    if lo.shape != (3,) or hi.shape != (3,):
        raise ValueError('bound_min / bound_max: three coordinates each')
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError('bound_min / bound_max must be finite')
    if not np.all(lo < hi):
        raise ValueError(f'bound_min {lo.tolist()} must be below bound_max {hi.tolist()} on every axis')
    return lo, hi


def _check_axes(shape):
    if len(shape) != 3 or not all(2 <= int(n) <= MAX_POINTS_PER_AXIS for n in shape):
        raise ValueError(f'grid {tuple(shape)}: three axes of 2..{MAX_POINTS_PER_AXIS} points each')


def marching_cubes(grid, threshold, bound_min, bound_max, valid=None):
    """grid [nx, ny, nz] fp32 device tensor -> (verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32), all on the
    grid's device.  An empty surface gives (0, 3) tensors.  Raises ValueError for a non-finite grid, threshold <= 0,
    bound_min >= bound_max on an axis or an axis outside 2..768 points.
    valid (None: every point, the path without a validity lattice): [nx, ny, nz] bool, True = observed.  Only cells whose
    eight corners are valid give triangles and only the edges around such cells vertices, so no surface appears where
    observed space meets unobserved space; a point that is not valid may hold anything, NaN included.  Normals stay
    central differences of the grid: within one lattice step of a point that is not valid they read its fill value."""
    if not torch.is_tensor(grid):
        raise ValueError('grid must be a torch tensor on the GPU')
    _check_axes(grid.shape)
    threshold = float(threshold)
    if not (threshold > 0 and math.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and > 0, got {threshold}')
    lo, hi = _bounds(bound_min, bound_max)
    return ops.marching_cubes(grid, threshold, lo, hi, device_table(grid.device), valid=valid)


def grid_axes(bound_min, bound_max, resolution, device):
    """The three coordinate vectors of the grid, as the kernels compute them: x0 + i * ((x1 - x0) / (n - 1)) in fp32."""
    lo, hi = _bounds(bound_min, bound_max)
    res = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)
    _check_axes(res)
    axes = []
    for a in range(3):
        h = (hi[a] - lo[a]) / np.float32(res[a] - 1)                       # fp32, as csrc/mcubes.hip
        axes.append(torch.arange(res[a], device=device, dtype=torch.float32) * float(h) + float(lo[a]))
    return axes


def _network(render_kwargs, network):
    if render_kwargs.get('ndc', False):
        raise ValueError('the model was trained in NDC space: its network input is not a world-space box (out of scope)')
    if network == 'fine':
        net = render_kwargs.get('network_fine')
        net = render_kwargs['network_fn'] if net is None else net
    elif network == 'coarse':
        net = render_kwargs['network_fn']
    else:
        raise ValueError(f"network must be 'fine' or 'coarse', got {network!r}")
    return net


def _query(render_kwargs, net, pts, dirs):
    """raw [P, C] of the model at pts [P, 3] seen along dirs [P, 3], through the model's own query function."""
    fn = render_kwargs['network_query_fn']
    raw = fn(pts[:, None, :], dirs if render_kwargs.get('use_viewdirs', True) else None, net)
    return raw.reshape(pts.shape[0], -1)


def density_grid(render_kwargs, bound_min, bound_max, resolution, network='fine', chunk=1 << 18):
    """sigma [nx, ny, nz] fp32 on the model's device: the network's raw density output (before the renderer's relu, which
    leaves the set sigma >= threshold > 0 unchanged) at the grid points, queried in chunks of `chunk` points with the
    constant view direction (0, 0, 1) (sigma does not depend on it), under torch.no_grad().  `network`: 'fine' (the fine
    network if the model has one) or 'coarse'.  resolution: an int or three point counts."""
    net = _network(render_kwargs, network)
    dev = next(net.parameters()).device
    xs, ys, zs = grid_axes(bound_min, bound_max, resolution, dev)
    nx, ny, nz = len(xs), len(ys), len(zs)
    n = nx * ny * nz
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be >= 1')
    sigma = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.no_grad():
        for s in range(0, n, chunk):
            idx = torch.arange(s, min(n, s + chunk), device=dev, dtype=torch.int64)
            i, r = idx // (ny * nz), idx % (ny * nz)
            pts = torch.stack([xs[i], ys[r // nz], zs[r % nz]], -1)
            dirs = torch.zeros_like(pts)
            dirs[:, 2] = 1.0
            sigma[s:s + idx.shape[0]] = _query(render_kwargs, net, pts, dirs)[:, 3]
    return sigma.view(nx, ny, nz)


def vertex_colors(render_kwargs, verts, normals, network='fine', chunk=1 << 18):
    """uint8 [V, 3] = sigmoid(raw[..., :3]) of the network at each vertex seen head-on (view direction = -normal)."""
    net = _network(render_kwargs, network)
    chunk = int(chunk)
    rgb = torch.empty((verts.shape[0], 3), device=verts.device, dtype=torch.uint8)
    with torch.no_grad():
        for s in range(0, verts.shape[0], chunk):
            raw = _query(render_kwargs, net, verts[s:s + chunk], -normals[s:s + chunk])
            rgb[s:s + chunk] = (torch.sigmoid(raw[:, :3]) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    return rgb


def remove_floaters(grid, threshold, largest=None, min_points=None, connectivity=6):
    """A copy of the sigma lattice `grid` [nx, ny, nz] (device) with every lattice point of a dropped component set to 0,
    which threshold > 0 makes "outside".  The components are those of the inside points (sigma >= threshold, the
    predicate of marching_cubes; csrc/components.hip).  largest = k keeps the k components with the most points (ties:
    the lower first point), min_points = m those of at least m points; a component must meet both where both are given.
    ValueError for no criterion, k < 1, m < 1, a connectivity other than 6 or 26, threshold <= 0.

    No lattice edge joins two different 6-components, so at connectivity 6 the crossing vertices of the kept components
    keep their positions bit for bit, and their faces with them.  Normals are central differences of sigma: one may
    differ where a dropped point lay within one lattice step of a kept vertex's edge."""
    if not torch.is_tensor(grid):
        raise ValueError('grid must be a torch tensor on the GPU')
    _check_axes(grid.shape)
    threshold = float(threshold)
    if not (threshold > 0 and math.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and > 0, got {threshold}')
    if connectivity not in ops.CONNECTIVITIES:
        raise ValueError(f'remove_floaters: connectivity must be 6 or 26, got {connectivity!r}')
    largest, min_points = ops.component_criteria('remove_floaters', largest, min_points, size_name='min_points')
    labels, sizes, _ = ops.grid_components(ops.grid_pack(grid, threshold), grid.shape, connectivity)
    keep = ops.component_keep_table(sizes.cpu().numpy(), largest, min_points)
    kept = torch.from_numpy(keep).to(grid.device)[labels.to(torch.int64)].bool()
    return torch.where(kept | (labels == 0), grid, torch.zeros((), device=grid.device, dtype=grid.dtype))


def extract_mesh(render_kwargs, bound_min, bound_max, resolution=256, threshold=10.0, colors=True, network='fine',
                 chunk=1 << 18, largest=None, min_points=None):
    """Mesh(verts, faces, normals, colors) of the surface sigma = threshold inside the box: marching_cubes(density_grid(...)),
    colours from vertex_colors() (uint8 [V, 3]), or None with colors=False.  largest / min_points (default None: the
    lattice goes to marching cubes as it is): remove_floaters() on the lattice first, at connectivity 6 -- the table cuts
    diagonal inside corners off separately, so the sheets of the mesh follow the 6-components of the inside points."""
    grid = density_grid(render_kwargs, bound_min, bound_max, resolution, network, chunk)
    if largest is not None or min_points is not None:
        grid = remove_floaters(grid, threshold, largest, min_points, connectivity=6)
    verts, faces, normals = marching_cubes(grid, threshold, bound_min, bound_max)
    rgb = vertex_colors(render_kwargs, verts, normals, network, chunk) if colors else None
    return Mesh(verts, faces, normals, rgb)


def fuse_depths(disp, poses, focal, bound_min, bound_max, resolution=256, trunc=None, masks=None, largest=None,
                min_points=None):
    """Mesh(verts, faces, normals, None) of the surface the depth maps see: ops.tsdf_fuse (csrc/tsdf.hip) fuses disp
    [V, H, W] (disparity = 1 / planar depth, as prepare.render_disparities returns it) of the cameras poses [V, 3, 4] into
    a truncated signed distance field on the lattice of the box, and marching cubes extracts its zero level set over the
    observed cells.  No threshold to choose: the iso value is 0.  trunc=None means four times the largest lattice step;
    masks [V, H, W] bool: False = ignore the pixel.

    The lattice handed to marching cubes is g = 1 - tsdf at threshold 1 (inside <=> g >= 1 <=> tsdf <= 0, the "threshold > 0,
    inside is >=" contract), with 0 at the points no view observed and valid = count > 0.  largest / min_points:
    remove_floaters(g, 1.0, ...) first (connectivity 6).  Normals point toward the cameras; within one lattice step of an
    unobserved point they read the fill value 0."""
    lo, hi = _bounds(bound_min, bound_max)
    res = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)
    _check_axes(res)
    if trunc is None:
        trunc = 4.0 * max(float((hi[a] - lo[a]) / np.float32(res[a] - 1)) for a in range(3))
    tsdf, count = ops.tsdf_fuse(disp, poses, focal, lo, hi, res, trunc, masks=masks)
    valid = count > 0
    g = torch.where(valid, 1.0 - tsdf, torch.zeros((), device=tsdf.device, dtype=tsdf.dtype))
    if largest is not None or min_points is not None:
        g = remove_floaters(g, 1.0, largest, min_points, connectivity=6)
    verts, faces, normals = marching_cubes(g, 1.0, lo, hi, valid=valid)
    return Mesh(verts, faces, normals, None)


SPREAD_LEVELS = (0.16, 0.5, 0.84)          # the quantiles behind max_spread: (z(0.84) - z(0.16)) / z(0.5)


def filtered_disparities(render_kwargs, hwf, poses, near, far, chunk=1 << 15, depth='expected', max_spread=None, min_agree=None,
                         max_violated=None, masks=None, tol=0.05):
    """(disp [V, H, W], poses [V, 3, 4] fp32 on disp's device, masks [V, H, W] bool or None, shares): what extract_mesh_tsdf
    hands to fuse_depths.  depth='expected': prepare.render_disparities; 'median': 1 / the median termination depth.
    max_spread=r keeps the pixels whose quantiles z(0.16), z(0.5), z(0.84) are finite with (z(0.84) - z(0.16)) / z(0.5) <= r
    (prepare.spread_mask); min_agree / max_violated keep those of prepare.consistency_mask of `disp` (a bound left None does
    not filter).  The filters are computed independently of one another and ANDed with `masks`; with none of them `masks`
    comes back as it is.  shares: per filter the share of pixels it masks ('spread', 'consistency'), for the record."""
    from . import prepare
    prepare._depth_kind('filtered_disparities', depth)
    depth_q = None
    if depth == 'median' or max_spread is not None:
        levels = SPREAD_LEVELS if max_spread is not None else (0.5,)
        depth_q = prepare.render_depth_quantiles(render_kwargs, hwf, poses, near, far, levels, chunk)
    if depth == 'median':
        disp = (1.0 / depth_q[..., levels.index(0.5)]).contiguous()
    else:
        disp = prepare.render_disparities(render_kwargs, hwf, poses, near, far, chunk=chunk)
    poses = torch.as_tensor(poses).to(device=disp.device, dtype=torch.float32)[:, :3, :4].contiguous()
    shares = {}
    keep = None
    if masks is not None:
        keep = torch.as_tensor(masks).to(disp.device) != 0
    if max_spread is not None:
        m = prepare.spread_mask(depth_q, max_spread)
        shares['spread'] = float((~m).float().mean().cpu()) if m.numel() else 0.0
        keep = m if keep is None else keep & m
    if min_agree is not None or max_violated is not None:
        m = prepare.consistency_mask(disp, poses, float(hwf[2]), tol=tol, min_agree=0 if min_agree is None else min_agree,
                                     max_violated=2 ** 31 - 1 if max_violated is None else max_violated)
        shares['consistency'] = float((~m).float().mean().cpu()) if m.numel() else 0.0
        keep = m if keep is None else keep & m
    if keep is None or (max_spread is None and min_agree is None and max_violated is None):
        return disp, poses, masks, shares
    return disp, poses, keep.contiguous(), shares


def extract_mesh_tsdf(render_kwargs, hwf, poses, near, far, bound_min, bound_max, resolution=256, trunc=None, colors=True,
                      network='fine', chunk=1 << 15, largest=None, min_points=None, masks=None, depth='expected', max_spread=None,
                      min_agree=None, max_violated=None):
    """Mesh of what the renderer sees rather than of what the network stores: prepare.render_disparities of every pose
    [V, 3, 4] (hwf = (H, W, focal); `chunk` rays at a time), fuse_depths() of those maps, colours from vertex_colors()
    (uint8 [V, 3]) or None with colors=False.  Compositing has integrated the fog along each ray away and the average over
    the views removes view-dependent floaters, so no sigma threshold is chosen.  Refuses NDC models (ValueError).

    depth / max_spread / min_agree / max_violated (defaults: today's result bit for bit) choose and filter the maps that are
    fused, filtered_disparities(): depth='median' fuses the median termination depth, which lies on a surface where the
    expected depth lies between two; max_spread drops the pixels whose ray does not see one surface; min_agree / max_violated
    drop those no other view confirms / another view sees through."""
    _network(render_kwargs, network)
    disp, poses, masks, _ = filtered_disparities(render_kwargs, hwf, poses, near, far, chunk, depth, max_spread, min_agree,
                                                 max_violated, masks)
    m = fuse_depths(disp, poses, float(hwf[2]), bound_min, bound_max, resolution, trunc, masks, largest, min_points)
    rgb = vertex_colors(render_kwargs, m.verts, m.normals, network) if colors else None
    return Mesh(m.verts, m.faces, m.normals, rgb)


def vertex_normals(mesh):
    """normals [V, 3] fp32 of `mesh` from its faces alone (ops.mesh_vertex_normals): area-weighted, outward for
    counter-clockwise faces.  What a mesh that was cropped, smoothed or simplified needs in place of the lattice normals."""
    return ops.mesh_vertex_normals(mesh.verts, mesh.faces)


def smooth(mesh, iters=10, lam=0.5, mu=-0.53):
    """Taubin smoothing (ops.mesh_smooth): a Mesh with the smoothed vertices, the faces and colours of `mesh` as they are
    and the normals recomputed from the faces.  lam shrinks, mu < -lam inflates again: lattice-frequency noise goes, the
    enclosed volume nearly stays (plain Laplacian smoothing, mu -> 0, shrinks the shape)."""
    verts = ops.mesh_smooth(mesh.verts, mesh.faces, iters, lam, mu)
    return Mesh(verts, mesh.faces, ops.mesh_vertex_normals(verts, mesh.faces), mesh.colors)


def simplify(mesh, cell, placement='quadric', dedupe=False, origin=None):
    """Simplification by vertex clustering (ops.mesh_cluster): every vertex in one cubic cell of edge `cell` (a bit grid that
    starts at `origin`, default the componentwise minimum of the vertices; 1..512 cells per axis) becomes one vertex, placed
    by `placement` ('quadric' or 'mean') inside that cell; faces that collapse are dropped; colours are the members' integer
    means; normals are recomputed from the faces.  No vertex moves by more than sqrt(3) cell.

    dedupe=False (the default) keeps a closed mesh closed: every directed edge stays balanced by its reverse, because a
    collapsed face contributes (a, a), (a, b), (b, a), which cancel.  dedupe=True also drops repeated faces (same directed
    cycle), which can break that balance."""
    verts, faces, colors, _ = ops.mesh_cluster(mesh.verts, mesh.faces, mesh.colors, origin, cell, placement, dedupe)
    return Mesh(verts, faces, ops.mesh_vertex_normals(verts, faces), colors)


def _view_poses(poses, device):
    return torch.as_tensor(poses).to(device=device, dtype=torch.float32)[:, :3, :4].contiguous()


def render_views(mesh, hwf, poses, near=1e-3, cull='none', colors=True):
    """(disp [V, H, W] fp32, face [V, H, W] int32, rgb [V, H, W, 3] uint8 or None) of `mesh` rasterised into the cameras poses
    [V, 3, >=4] (ops.mesh_rasterize, csrc/raster.hip; hwf = (H, W, focal)): the inverse of prepare.render_disparities, in its
    conventions, so the maps compare pixel by pixel with the field's own renders.  disp is 0 and face -1 where the mesh does
    not cover the pixel.  rgb interpolates mesh.colors (None with colors=False or a mesh without colours).  cull='back' drops
    the faces seen from inside.  There is no near-plane clipping: a face with a vertex nearer than `near` is dropped whole."""
    c = mesh.colors if colors else None
    return ops.mesh_rasterize(mesh.verts, mesh.faces, _view_poses(poses, mesh.verts.device), int(hwf[0]), int(hwf[1]),
                              float(hwf[2]), near=near, cull=cull, colors=c)


def visible_faces(mesh, hwf, poses, near=1e-3, cull='none', chunk=32):
    """bool [F] on the mesh's device: the faces that win at least one pixel of at least one of the views poses [V, 3, >=4]
    (render_views, `chunk` views at a time).  Interior sheets and back shells of a sigma level set win none."""
    F = int(mesh.faces.shape[0])
    seen = torch.zeros(F, device=mesh.verts.device, dtype=torch.bool)
    poses = _view_poses(poses, mesh.verts.device)
    for s in range(0, poses.shape[0], max(1, int(chunk))):
        face = render_views(mesh, hwf, poses[s:s + int(chunk)], near, cull, colors=False)[1]
        seen[face[face >= 0].to(torch.int64)] = True
    return seen


def keep_faces(mesh, keep):
    """The mesh with only the faces keep [F] bool marks (torch plumbing): the faces keep their order, the vertices no kept face
    references are dropped and the others keep theirs, normals and colours are carried over."""
    keep = torch.as_tensor(keep, device=mesh.faces.device)
    if keep.dtype != torch.bool or tuple(keep.shape) != (mesh.faces.shape[0],):
        raise ValueError(f'keep_faces: keep must be bool [{mesh.faces.shape[0]}], got {keep.dtype} {tuple(keep.shape)}')
    faces = mesh.faces[keep]
    used = torch.zeros(mesh.verts.shape[0], device=mesh.verts.device, dtype=torch.bool)
    used[faces.reshape(-1).to(torch.int64)] = True
    new = (torch.cumsum(used, 0) - 1).to(torch.int32)
    pick = lambda a: None if a is None else a[used].contiguous()
    return Mesh(pick(mesh.verts), new[faces.to(torch.int64)].contiguous(), pick(mesh.normals), pick(mesh.colors))


def cast_rays(mesh, rows, grid=None):
    """(face [B] int32, depth [B] fp32, disparity [B] fp32) of run.render_rays' own ray rows [B, 8 | 11] (origin, direction,
    near, far, ...) cast against `mesh` (ops.mesh_cast_rays, csrc/mesh_raycast.hip): the first face hit between near and far,
    -1 for none; depth = the ray parameter of the hit, which for the rows of get_rays (camera z = -1) is the planar depth, +inf
    for none; disparity = 1 / depth and 0 for none -- the conventions of render_views and prepare.render_disparities."""
    rows = torch.as_tensor(rows)
    if rows.dim() != 2 or rows.shape[1] not in (8, 11) or rows.dtype != torch.float32:
        raise ValueError(f'cast_rays: rows must be fp32 [B, 8] or [B, 11], got {rows.dtype} {tuple(rows.shape)}')
    rows = rows.detach().to(mesh.verts.device)
    face, depth = ops.mesh_cast_rays(rows[:, 0:3].contiguous(), rows[:, 3:6].contiguous(), mesh.verts, mesh.faces,
                                     tmin=rows[:, 6].contiguous(), tmax=rows[:, 7].contiguous(), grid=grid)
    return face, depth, torch.where(face >= 0, (1.0 / depth.double()).float(), torch.zeros_like(depth))


def cast_views(mesh, hwf, poses, near, far, colors=True):
    """(disp [V, H, W] fp32, face [V, H, W] int32, rgb [V, H, W, 3] uint8 or None) of `mesh` ray cast into the cameras poses
    [V, 3, >=4]: render_views' outputs in render_views' conventions, from one ray per pixel centre (ops.get_rays) instead of the
    rasteriser.  A face that crosses the near plane is still seen beyond it, where render_views drops it whole.  rgb is the
    barycentric mean of the hit face's vertex colours, rounded to the nearest byte (None with colors=False or a mesh without
    colours).  The two renderers agree except along silhouettes and shared edges: the rasteriser snaps vertices to 8 sub-pixel
    bits and fills by the top-left rule, the ray cast does neither."""
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    dev = mesh.verts.device
    poses = _view_poses(poses, dev)
    V = int(poses.shape[0])
    want_rgb = colors and mesh.colors is not None
    if V == 0:
        return (torch.zeros((0, H, W), device=dev), torch.zeros((0, H, W), device=dev, dtype=torch.int32),
                torch.zeros((0, H, W, 3), device=dev, dtype=torch.uint8) if want_rgb else None)
    rays = [ops.get_rays(H, W, focal, p) for p in poses]
    o = torch.stack([r[0] for r in rays]).reshape(-1, 3)
    d = torch.stack([r[1] for r in rays]).reshape(-1, 3)
    out = ops.mesh_cast_rays(o, d, mesh.verts, mesh.faces, tmin=float(near), tmax=float(far), return_bary=want_rgb)
    face, depth = out[0], out[1]
    hit = face >= 0
    disp = torch.where(hit, (1.0 / depth.double()).float(), torch.zeros_like(depth)).reshape(V, H, W)
    rgb = None
    if want_rgb:
        bary = torch.nan_to_num(out[2])
        corner = mesh.faces[face.clamp(min=0).to(torch.int64)].to(torch.int64)             # [B, 3]
        c = mesh.colors[corner].to(torch.float32)                                        # [B, 3 corners, 3 channels]
        w = torch.stack([1.0 - bary[:, 0] - bary[:, 1], bary[:, 0], bary[:, 1]], 1)
        mixed = (c * w[:, :, None]).sum(1)
        rgb = torch.where(hit[:, None], (mixed + 0.5).floor().clamp(0, 255), torch.zeros_like(mixed)).to(torch.uint8).reshape(V, H, W, 3)
    return disp, face.reshape(V, H, W), rgb


def fibonacci_directions(count):
    """[count, 3] fp32 numpy: the spherical Fibonacci set z_i = 1 - (2 i + 1) / count, phi_i = pi (1 + sqrt 5) (i + 1/2),
    (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), computed in fp64 and rounded once.  Nothing is random."""
    if isinstance(count, bool) or int(count) != count or not 1 <= int(count) <= ops.MESH_OPENNESS_MAX_DIRECTIONS:
        raise ValueError(f'fibonacci_directions: count must be an integer in 1..{ops.MESH_OPENNESS_MAX_DIRECTIONS}, got {count!r}')
    i = np.arange(int(count), dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / int(count)
    phi = np.pi * (1.0 + np.sqrt(5.0)) * (i + 0.5)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


def _openness_args(mesh, directions, max_dist):
    if not torch.is_tensor(directions):
        directions = fibonacci_directions(directions) if np.isscalar(directions) else np.asarray(directions, np.float32)
        directions = torch.from_numpy(np.ascontiguousarray(directions))
    directions = directions.to(device=mesh.verts.device, dtype=torch.float32).contiguous()
    return directions, float('inf') if max_dist is None else float(max_dist)


def face_openness(mesh, directions=32, max_dist=None):
    """(front_open, front_total, back_open, back_total), int32 [F] each (ops.mesh_face_openness, csrc/mesh_raycast.hip): of the
    directions on a face's front side (N . d > 0, N the face normal of counter-clockwise faces) and on its back side, how many
    see nothing of the mesh within max_dist (None: no limit) from the face's centroid.  directions: a count (the spherical
    Fibonacci set of that size) or [K, 3] directions, K <= 255.  An exterior face of a closed surface has every front direction
    open; a face of an interior shell has none on either side."""
    d, far = _openness_args(mesh, directions, max_dist)
    return ops.mesh_face_openness(mesh.verts, mesh.faces, d, max_dist=far)


def drop_interior(mesh, directions=32, two_sided=True, max_dist=None):
    """The mesh without the faces that see nothing but mesh (face_openness, keep_faces): a face stays iff at least one direction
    is open on either side (two_sided=True: right for level sets whose orientation is not trusted, and for open sheets) or on
    its front side (two_sided=False: also drops the inner wall of a thick shell).  Unlike keeping the faces some camera saw
    (visible_faces), exterior surface that no camera happened to see stays."""
    fo, _, bo, _ = face_openness(mesh, directions, max_dist)
    return keep_faces(mesh, (fo + bo > 0) if two_sided else (fo > 0))


# ---- topology (csrc/mesh_topology.hip): which faces belong together, is the surface closed, where are its holes ----------------
TOPOLOGY_COLUMNS = ('faces', 'vertices', 'edges', 'boundary_edges', 'non_manifold_edges', 'inconsistent_edges')


def topology(mesh, connectivity='edge'):
    """A report on the surface as a dict: the totals of TOPOLOGY_COLUMNS (vertices: those some non-degenerate face references),
    `components` (their number) and `per_component` (a list of dicts with the same columns plus closed / oriented / euler /
    genus, in label order = by lowest face), `degenerate_faces`, `closed` (no boundary and no non-manifold edge), `oriented` (no
    edge whose two faces run it the same way, none with three or more faces), `euler` = V - E + F, `genus` = (2 - euler) / 2 of
    a component where it is closed and oriented, else None (the mesh's genus: the sum over its components, None if any is
    None), `loops` and `closed_loops` (boundary_loops).  connectivity 'edge' or 'vertex' (ops.mesh_components)."""
    V = int(mesh.verts.shape[0])
    labels, table = ops.mesh_components(mesh.faces, V, connectivity)
    loops = ops.mesh_boundary_loops(mesh.faces, V)
    t = table.cpu().numpy().astype(np.int64).reshape(-1, 6)

    def describe(row):
        d = dict(zip(TOPOLOGY_COLUMNS, (int(x) for x in row)))
        d['closed'] = d['boundary_edges'] == 0 and d['non_manifold_edges'] == 0
        d['oriented'] = d['inconsistent_edges'] == 0 and d['non_manifold_edges'] == 0
        d['euler'] = d['vertices'] - d['edges'] + d['faces']
        return d

    per = [describe(r) for r in t]
    for d in per:
        d['genus'] = (2 - d['euler']) // 2 if d['closed'] and d['oriented'] else None
    out = describe(t.sum(0))
    out['genus'] = sum(d['genus'] for d in per) if all(d['genus'] is not None for d in per) else None
    out.update(components=len(per), per_component=per, degenerate_faces=int((labels == 0).sum()),
               loops=int(loops.first.shape[0]), closed_loops=int(loops.closed.sum()) if loops.closed.shape[0] else 0)
    return out


def keep_components(mesh, largest=None, min_faces=None, containing=None, connectivity='edge'):
    """The mesh with only the faces of the kept components (ops.mesh_components, keep_faces): largest = k keeps the k
    components with the most faces (ties: the lower label = the lower first face), min_faces = m those of at least m faces, a
    component must meet both where both are given (ops.component_criteria / component_keep_table, as remove_floaters on the
    lattice); containing: [N, 3] points, the component of each point's closest face (ops.mesh_closest_point) is kept in any
    case.  Kept faces and vertices keep their order and their bits; degenerate faces go.  ValueError for no criterion."""
    largest, min_faces = ops.component_criteria('keep_components', largest, min_faces, other=containing is not None,
                                                size_name='min_faces')
    labels, table = ops.mesh_components(mesh.faces, int(mesh.verts.shape[0]), connectivity)
    also = None
    if containing is not None and mesh.faces.shape[0]:
        pts = torch.as_tensor(containing, dtype=torch.float32).reshape(-1, 3).to(mesh.verts.device).contiguous()
        if pts.shape[0]:
            face = ops.mesh_closest_point(pts, mesh.verts, mesh.faces)[0]
            also = labels[face[face >= 0].to(torch.int64)].cpu().numpy()
    keep = ops.component_keep_table(table[:, 0].cpu().numpy(), largest, min_faces, also)
    return keep_faces(mesh, torch.from_numpy(keep).to(mesh.faces.device)[labels.to(torch.int64)].bool())


VOXEL_MODES = ('surface', 'solid', 'both')


def voxelize(mesh, bmin, bmax, cells, mode='both', axes='majority'):
    """(grid, report): `mesh` as a bitgrid.BitGrid on the box [bmin, bmax] cut into `cells` (ops.mesh_voxelize_surface /
    mesh_voxelize_solid, csrc/mesh_voxel.hip).  mode 'surface': the cells the faces touch, conservatively (every point of a face
    that the renderer's cell lookup places in the box lies in a set cell); 'solid': the cells whose centres are inside, by column
    parity along `axes` ('x', 'y', 'z', or 'majority' of the three -- the one to use on meshes with holes, such as TSDF meshes);
    'both': the OR of the two.  report: a dict of `dropped` (faces left out: non-finite or, for 'solid', beyond the guard band;
    the larger of the two counts under 'both'), `odd_columns` (three integers, the leak diagnostic of 'solid': columns of odd
    parity per axis -- zero for a closed mesh that no column ends inside; None for 'surface'), `count` (set cells), `volume`
    (count x the volume of a cell) and `cells`.  The grid is a plain BitGrid: Region.from_mesh and OccupancyGrid.from_mesh give
    it a meaning."""
    from . import bitgrid
    if mode not in VOXEL_MODES:
        raise ValueError(f'voxelize: mode must be one of {VOXEL_MODES}, got {mode!r}')
    if axes not in ops.VOXEL_AXES:
        raise ValueError(f'voxelize: axes must be one of {ops.VOXEL_AXES}, got {axes!r}')
    dev = mesh.verts.device
    cells = bitgrid._cells(cells)
    grid = bitgrid.BitGrid(bmin, bmax, cells, torch.zeros(ops.occupancy_words(cells), device=dev, dtype=torch.int32))
    words, dropped, odd = None, 0, None
    if mode in ('surface', 'both'):
        words, dropped = ops.mesh_voxelize_surface(mesh.verts, mesh.faces, grid.box(), cells)
    if mode in ('solid', 'both'):
        w, odd, d = ops.mesh_voxelize_solid(mesh.verts, mesh.faces, grid.box(), cells, axes)
        words = w if words is None else words | w
        dropped = max(dropped, d)
    grid = bitgrid.BitGrid(grid.bmin, grid.bmax, cells, words)
    count = grid.count()
    cell_volume = float(np.prod((grid.bmax.astype(np.float64) - grid.bmin.astype(np.float64)) / np.asarray(cells, np.float64)))
    return grid, {'dropped': int(dropped), 'odd_columns': None if odd is None else [int(o) for o in odd], 'count': count,
                  'volume': count * cell_volume, 'cells': cells}


def boundary_loops(mesh):
    """ops.MeshBoundaryLoops(loop_of [3F], next [3F], first [L], sizes [L], closed [L]) of the mesh's boundary: the holes of a
    surface that should be closed, the rim of one that is a sheet.  See ops.mesh_boundary_loops."""
    return ops.mesh_boundary_loops(mesh.faces, int(mesh.verts.shape[0]))


def close_holes(mesh, max_edges=64):
    """(mesh', capped, left): the mesh with every closed boundary loop of 3..max_edges edges capped by a fan round the loop's
    centroid (ops.mesh_cap_loops), the number of loops capped and the number left open.  The caps are appended: the old
    vertices, faces, colours and normals keep their rows bit for bit; a new vertex takes the mean colour of its loop, and
    where the mesh carries normals its row is that of ops.mesh_vertex_normals of the capped mesh.  The new faces are wound
    against the boundary, so a consistently oriented mesh stays so.

    What a centroid fan is NOT: a hole filler for large or strongly non-planar holes.  The centroid of a long or bent loop can
    lie far from any sensible surface (outside the shape for a C-shaped rim), the fan can fold over itself or cut through the
    mesh, and its triangles are slivers when the loop is long.  It is right for the small, nearly flat cuts that dropping
    unseen or interior faces leaves; max_edges is there to keep it to those, and loops that touch themselves at a vertex
    (not closed) are never capped."""
    new_v, new_c, new_f, capped = ops.mesh_cap_loops(mesh.verts, mesh.faces, mesh.colors, max_edges)
    n_capped = int(capped.sum()) if capped.shape[0] else 0
    left = int(capped.shape[0]) - n_capped
    if n_capped == 0:
        return mesh, 0, left
    verts = torch.cat([mesh.verts, new_v]).contiguous()
    faces = torch.cat([mesh.faces, new_f]).contiguous()
    colors = None if mesh.colors is None else torch.cat([mesh.colors, new_c]).contiguous()
    normals = mesh.normals
    if normals is not None:
        normals = torch.cat([normals, ops.mesh_vertex_normals(verts, faces)[mesh.verts.shape[0]:]]).contiguous()
    return Mesh(verts, faces, normals, colors), n_capped, left


# ---- signed distance (csrc/mesh_sdf.hip): which side of the surface, how far, and the mesh extracted again from that field ------
SDF_DEFAULT_BAND_STEPS = 3.0
REMESH_MIN_BAND_STEPS = 2.0


def signed_distance(mesh, points, max_dist=None):
    """(sdist [N] fp32, face [N] int32, point [N, 3] fp32) of points [N, 3] against the mesh (ops.mesh_signed_distance): the
    distance to the closest point of the surface, negative inside a closed mesh with outward faces (marching_cubes', close_holes'
    orientation); max_dist: points farther than it get face -1 and NaN.  On an open or inconsistently oriented mesh the sign is
    that of the closest feature's pseudonormal and means what that mesh's orientation means: topology() says which it is."""
    pts = torch.as_tensor(points, dtype=torch.float32).reshape(-1, 3).to(mesh.verts.device).contiguous()
    return ops.mesh_signed_distance(pts, mesh.verts, mesh.faces, max_dist=max_dist)


def _largest_step(bound_min, bound_max, resolution):
    return float(max(ops.mesh_lattice(bound_min, bound_max, resolution)[1]))


def sdf_grid(mesh, bound_min, bound_max, resolution, band=None):
    """(sd [nx, ny, nz] fp32, valid [nx, ny, nz] bool): the signed distance of the mesh on the lattice of grid_axes(bound_min,
    bound_max, resolution) within `band` of the surface (None: three times the largest lattice step); valid = within the band,
    sd is NaN elsewhere.  One lattice-mode launch (ops.mesh_signed_distance_lattice): the lattice points are never written out,
    and a point far from the surface costs the few cells it takes to know that."""
    lo, hi = _bounds(bound_min, bound_max)
    if band is None:
        band = SDF_DEFAULT_BAND_STEPS * _largest_step(lo, hi, resolution)
    sd, face = ops.mesh_signed_distance_lattice(mesh.verts, mesh.faces, lo, hi, resolution, max_dist=band)
    return sd, face >= 0


def remesh(mesh, resolution=256, offset=0.0, band=None, bound_min=None, bound_max=None):
    """The level set sdist = offset of the mesh's signed distance, extracted again by marching cubes on `resolution` lattice
    points per axis: a closed, evenly tessellated Mesh (no colours: colors_from_views / bake_texture give it some; normals from
    its faces) in place of whatever drop_interior, keep_components and close_holes left -- centroid fans, slivers, sheets that
    touch.  offset > 0 grows the shape, < 0 shrinks it.  The lattice handed to marching_cubes is band - sd where sd is known and
    0 elsewhere, the threshold band - offset, with sdf_grid's valid lattice: "threshold > 0, inside is >=", as fuse_depths.
    band None: three lattice steps; ValueError unless |offset| + 2 steps <= band (every corner of a cell the level set crosses
    must lie within the band).  The default box is the vertex bounds grown by band.  The sign needs a closed, consistently
    oriented input (topology()); on an open sheet the result is the sheet's two-sided band only where the pseudonormal sign
    happens to flip, which is not a use of this function."""
    res = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(n) for n in resolution)
    _check_axes(res)
    offset = float(offset)
    if not math.isfinite(offset):
        raise ValueError(f'remesh: offset must be finite, got {offset}')
    if int(mesh.verts.shape[0]) == 0 or int(mesh.faces.shape[0]) == 0:
        raise ValueError('remesh: an empty mesh has no distance field')
    if (bound_min is None) != (bound_max is None):
        raise ValueError('remesh: bound_min and bound_max go together')
    if bound_min is None:
        vlo, vhi = (t.cpu().numpy().astype(np.float64) for t in (mesh.verts.amin(0), mesh.verts.amax(0)))
        if band is None:                                      # band = 3 steps of the box grown by band: solve for band
            if min(res) <= 2 * SDF_DEFAULT_BAND_STEPS + 1:
                raise ValueError(f'remesh: resolution {res} leaves no room for a band of {SDF_DEFAULT_BAND_STEPS} steps on each side')
            grow = max(SDF_DEFAULT_BAND_STEPS * (vhi[a] - vlo[a]) / (res[a] - 1 - 2 * SDF_DEFAULT_BAND_STEPS) for a in range(3))
            grow = max(grow, 1e-6 * max(1.0, float(np.abs(np.concatenate([vlo, vhi])).max())))        # a flat mesh still gets a box
        else:
            grow = float(band)
        if not (math.isfinite(grow) and grow > 0):
            raise ValueError(f'remesh: band must be finite and > 0, got {band!r}')
        bound_min, bound_max = vlo - grow, vhi + grow
    lo, hi = _bounds(bound_min, bound_max)
    step = _largest_step(lo, hi, res)
    band = SDF_DEFAULT_BAND_STEPS * step if band is None else float(band)
    if not (math.isfinite(band) and abs(offset) + REMESH_MIN_BAND_STEPS * step <= band):
        raise ValueError(f'remesh: |offset| + {REMESH_MIN_BAND_STEPS:g} lattice steps = {abs(offset) + REMESH_MIN_BAND_STEPS * step:g} '
                         f'must not exceed band = {band:g}')
    sd, valid = sdf_grid(mesh, lo, hi, res, band)
    g = torch.where(valid, band - sd, torch.zeros_like(sd)).contiguous()
    verts, faces, _ = marching_cubes(g, band - offset, lo, hi, valid=valid.contiguous())
    normals = ops.mesh_vertex_normals(verts, faces) if verts.shape[0] else verts.clone()
    return Mesh(verts, faces, normals, None)


def margin_cells(mesh, bmin, bmax, cells, margin):
    """int32 words (the bit grid of `cells` cells on [bmin, bmax]) of the cells whose CENTRE lies within |margin| of the mesh's
    surface: the metric margin of Region.from_mesh / OccupancyGrid.from_mesh.  One lattice-mode launch with max_dist = |margin|
    on the fp32 centres fp32(bmin + w / 2) .. fp32(bmax - w / 2), w = (bmax - bmin) / cells in fp64, computed once here; in the
    band <=> face >= 0; packed by ops.grid_pack.  ValueError for a margin that is not finite, and (the lattice needs two points
    per axis) for an axis of one cell."""
    from . import bitgrid
    cells = bitgrid._cells(cells)
    margin = float(margin)
    if not math.isfinite(margin):
        raise ValueError(f'margin must be finite, got {margin}')
    if min(cells) < 2:
        raise ValueError(f'a margin needs at least two cells per axis, got {cells}')
    lo, hi = _bounds(bmin, bmax)
    w = (hi.astype(np.float64) - lo.astype(np.float64)) / np.asarray(cells, np.float64)
    first, last = (lo.astype(np.float64) + w / 2).astype(np.float32), (hi.astype(np.float64) - w / 2).astype(np.float32)
    _, face = ops.mesh_signed_distance_lattice(mesh.verts, mesh.faces, first, last, cells, max_dist=abs(margin))
    return ops.grid_pack((face >= 0).to(torch.float32), 0.5)


def apply_margin(words, mesh, bmin, bmax, cells, margin):
    """words with the cells of margin_cells set (margin > 0) or cleared (margin < 0); margin None or 0: words as they are."""
    if margin is None or float(margin) == 0.0:
        return words
    m = margin_cells(mesh, bmin, bmax, cells, margin)
    return (words | m) if float(margin) > 0 else (words & ~m)


Texture = collections.namedtuple('Texture', ['image', 'uv', 'seen', 'texels'])


def atlas_layout(n_faces, texels):
    """((Ht, Wt, 3), uv [F, 3, 2] fp32 numpy): the shape of the texture atlas of a mesh of n_faces faces at `texels` texels along a
    face's leg (1..32) and the texture coordinates of every face corner in OBJ convention, u = x / Wt, v = 1 - y / Ht of the
    continuous texel position (texel centres at integer + 1/2).  The layout is csrc/texture.hip's, a pure integer function of
    (F, texels): faces 2k and 2k + 1 share block k of side S = texels + 3, the blocks lie row-major, ceil(sqrt(ceil(F / 2))) per
    row; face 2k has its corners at (1/2, 1/2), (texels + 1/2, 1/2), (1/2, texels + 1/2) of the block, face 2k + 1 the same
    reflected through the block's centre.  A bilinear lookup inside a face's UV triangle reads only texels that face owns.
    ValueError for texels outside 1..32 or a texture side over 16,384.  Host code."""
    Ht, Wt, Bx, _, S = ops.texture_layout(n_faces, texels)
    F, n = int(n_faces), int(texels)
    f = np.arange(F, dtype=np.int64)
    k = f // 2
    by, bx = k // max(Bx, 1), k % max(Bx, 1)
    upper = (f % 2 == 1)[:, None]
    a, b = np.array([0.0, n, 0.0])[None], np.array([0.0, 0.0, n])[None]
    x = np.where(upper, ((bx + 1) * S)[:, None] - 0.5 - a, (bx * S)[:, None] + 0.5 + a)
    y = np.where(upper, ((by + 1) * S)[:, None] - 0.5 - b, (by * S)[:, None] + 0.5 + b)
    uv = np.stack([x / float(max(Wt, 1)), 1.0 - y / float(max(Ht, 1))], -1).astype(np.float32)
    return (Ht, Wt, 3), uv


def _texel_points(mesh, texels, idx):
    """(points, unit normals) [K, 3] fp32 of the texels idx [K] (flat y * Wt + x, all owned) of the atlas of `mesh`, in torch on
    the mesh's device: the sample points of csrc/texture.hip rounded to fp32, for the field query of bake_texture."""
    F = int(mesh.faces.shape[0])
    _, Wt, Bx, _, S = ops.texture_layout(F, texels)
    n = int(texels)
    Y, X = idx // Wt, idx % Wt
    bx, by = X // S, Y // S
    i, j = X - bx * S, Y - by * S
    upper = i + j > S - 1
    face = 2 * (by * Bx + bx) + upper.to(torch.int64)
    i, j = torch.where(upper, S - 1 - i, i), torch.where(upper, S - 1 - j, j)
    inner = i + j < n
    m = (i - j + n).clamp(0, 2 * n)
    l1 = torch.where(inner, i.double() / n, m.double() / (2 * n))
    l2 = torch.where(inner, j.double() / n, (2 * n - m).double() / (2 * n))
    l0 = torch.where(inner, (1.0 - l1) - l2, torch.zeros_like(l1))
    fv = mesh.verts.double()[mesh.faces.to(torch.int64)[face]]                          # [K, 3, 3]
    p = (l0[:, None] * fv[:, 0] + l1[:, None] * fv[:, 1]) + l2[:, None] * fv[:, 2]
    nrm = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True).clamp_min(1e-300)
    return p.float().contiguous(), nrm.float().contiguous()


def _byte_images(images, device):
    """images [V, H, W, 3] as uint8 on `device`: uint8 as it is, floats in 0..1 by floor(255 x + 1/2) clamped."""
    im = torch.as_tensor(images).to(device)
    if im.dtype != torch.uint8:
        im = (im.float() * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)
    return im.contiguous()


def bake_texture(mesh, hwf, poses, images, texels=8, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None, render_kwargs=None,
                 network='fine', chunk=1 << 18, verbose=True):
    """Texture(image [Ht, Wt, 3] uint8, uv [F, 3, 2] fp32 numpy, seen [Ht, Wt] bool, texels) of `mesh` baked from images [V, H, W, 3]
    (uint8, or floats in 0..1) of the cameras poses [V, 3, >=4], hwf = (H, W, focal): the mesh is rasterised into the views for
    its own disparities (render_views, cull off: a back face occludes too), then ops.mesh_bake_atlas blends per texel the views
    that see it (csrc/texture.hip; atlas_layout for the layout).  seen = a view contributed (wsum > 0).  Texels no view sees
    hold 0, or with render_kwargs the field's colour at the texel's point seen head-on (view direction = -face normal, the rule
    of vertex_colors, `chunk` points at a time).  Prints the unseen share of the owned texels (verbose)."""
    dev = mesh.verts.device
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    p = _view_poses(poses, dev)
    im = _byte_images(images, dev)
    m = None if masks is None else torch.as_tensor(masks).to(dev).bool().contiguous()
    disp = ops.mesh_rasterize(mesh.verts, mesh.faces, p, H, W, focal, near=near, cull='none')[0]
    rgb, wsum, best = ops.mesh_bake_atlas(mesh.verts, mesh.faces, texels, im, disp, p, focal, near=near, tol=tol, cull=cull, mode=mode,
                                          masks=m)
    seen = wsum > 0
    F = int(mesh.faces.shape[0])
    Ht, Wt, Bx, _, S = ops.texture_layout(F, texels)
    owned = _owned_texels(F, texels, dev)
    unseen = owned & ~seen
    n_owned, n_unseen = int(owned.sum()), int(unseen.sum())
    if render_kwargs is not None and n_unseen:
        net = _network(render_kwargs, network)
        idx = torch.nonzero(unseen.reshape(-1)).reshape(-1)
        flat = rgb.reshape(-1, 3)
        with torch.no_grad():
            for s in range(0, idx.shape[0], int(chunk)):
                pts, nrm = _texel_points(mesh, texels, idx[s:s + int(chunk)])
                raw = _query(render_kwargs, net, pts, -nrm)
                flat[idx[s:s + int(chunk)]] = (torch.sigmoid(raw[:, :3]) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    if verbose:
        print(f'texture {Ht} x {Wt} at {int(texels)} texels per leg: {n_owned} owned texels, {n_unseen} seen by no view '
              f'({n_unseen / max(n_owned, 1):.4f})' + (', filled from the field' if render_kwargs is not None and n_unseen else ''))
    return Texture(rgb, atlas_layout(F, texels)[1], seen, int(texels))


def _owned_texels(n_faces, texels, device):
    """bool [Ht, Wt]: the texels of the atlas that a face owns."""
    Ht, Wt, Bx, _, S = ops.texture_layout(n_faces, texels)
    Y, X = torch.meshgrid(torch.arange(Ht, device=device), torch.arange(Wt, device=device), indexing='ij')
    bx, by = X // S, Y // S
    upper = (X - bx * S) + (Y - by * S) > S - 1
    return 2 * (by * Bx + bx) + upper.to(torch.int64) < int(n_faces)


def colors_from_views(mesh, hwf, poses, images, near=1e-3, tol=0.05, cull='back', mode='blend', masks=None):
    """A Mesh whose vertex colours are baked from the views at the vertices with mesh.normals (ops.mesh_bake_points; the
    arguments of bake_texture): the colour the cameras saw where the vertex IS, not the field's answer at a point that smoothing
    or clustering has moved off its surface.  A vertex that no view sees keeps its old colour (0 for a mesh without colours)."""
    dev = mesh.verts.device
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    p = _view_poses(poses, dev)
    m = None if masks is None else torch.as_tensor(masks).to(dev).bool().contiguous()
    disp = ops.mesh_rasterize(mesh.verts, mesh.faces, p, H, W, focal, near=near, cull='none')[0]
    rgb, wsum, _ = ops.mesh_bake_points(mesh.verts, mesh.normals.contiguous(), _byte_images(images, dev), disp, p, focal, near=near,
                                        tol=tol, cull=cull, mode=mode, masks=m)
    old = mesh.colors if mesh.colors is not None else torch.zeros_like(rgb)
    return Mesh(mesh.verts, mesh.faces, mesh.normals, torch.where((wsum > 0)[:, None], rgb, old))


def render_textured(mesh, texture, hwf, poses, near=1e-3, cull='none'):
    """(disp [V, H, W] fp32, face [V, H, W] int32, rgb [V, H, W, 3] uint8) of `mesh` with `texture` (bake_texture) in the cameras
    poses [V, 3, >=4]: render_views for the geometry, ops.mesh_texture_resolve for the colour (the atlas read bilinearly at the
    perspective-correct position inside the winning face).  rgb is 0 where the mesh does not cover the pixel."""
    dev = mesh.verts.device
    p = _view_poses(poses, dev)
    focal = float(hwf[2])
    disp, face, _ = ops.mesh_rasterize(mesh.verts, mesh.faces, p, int(hwf[0]), int(hwf[1]), focal, near=near, cull=cull)
    image = torch.as_tensor(texture.image).to(dev).contiguous()
    return disp, face, ops.mesh_texture_resolve(face, mesh.verts, mesh.faces, image, texture.texels, p, focal, near=near)


def frustum_bounds(poses, hwf, near, far):
    """(bound_min, bound_max) float32 [3] each: the axis-aligned box of every camera's view frustum between near and far.
    poses [N, 3, >=4] camera-to-world (run.py's convention: x right, y up, looking down -z); hwf = (H, W, focal); the
    frustum is spanned by the rays of the corner pixels (get_rays: direction ((i - W/2) / f, -(j - H/2) / f, -1), i in
    {0, W - 1}, j in {0, H - 1}) at depth near and far.  A default box; users usually crop tighter."""
    P = np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses, dtype=np.float64)
    if P.ndim == 2:
        P = P[None]
    H, W, f = float(hwf[0]), float(hwf[1]), float(hwf[2])
    if not (near < far):
        raise ValueError('near must be < far')
    i = np.array([0.0, W - 1.0, 0.0, W - 1.0])
    j = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    d_cam = np.stack([(i - W * 0.5) / f, -(j - H * 0.5) / f, -np.ones(4)], -1)            # [4, 3]
    d = np.einsum('kc,nrc->nkr', d_cam, P[:, :3, :3])                                     # [N, 4, 3]
    o = P[:, None, :3, 3]
    corners = np.concatenate([o + d * float(near), o + d * float(far)], 1).reshape(-1, 3)
    return corners.min(0).astype(np.float32), corners.max(0).astype(np.float32)


def save_ply(path, mesh):
    """Binary little-endian PLY: float x y z, float nx ny nz, uchar red green blue (when mesh.colors is not None), and
    `uchar int` face lists."""
    v = np.ascontiguousarray(mesh.verts.detach().cpu().numpy() if torch.is_tensor(mesh.verts) else mesh.verts, '<f4')
    nrm = np.ascontiguousarray(mesh.normals.detach().cpu().numpy() if torch.is_tensor(mesh.normals) else mesh.normals,
                               '<f4')
    f = np.ascontiguousarray(mesh.faces.detach().cpu().numpy() if torch.is_tensor(mesh.faces) else mesh.faces, '<i4')
    c = mesh.colors
    if c is not None:
        c = np.ascontiguousarray(c.detach().cpu().numpy() if torch.is_tensor(c) else c, np.uint8)
    vfields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    if c is not None:
        vfields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vert = np.empty(v.shape[0], dtype=vfields)
    vert['x'], vert['y'], vert['z'] = v[:, 0], v[:, 1], v[:, 2]
    vert['nx'], vert['ny'], vert['nz'] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if c is not None:
        vert['red'], vert['green'], vert['blue'] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(f.shape[0], dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    face['n'] = 3
    face['v'] = f
    head = ['ply', 'format binary_little_endian 1.0', 'comment mvip_nerf_amd.mesh', f'element vertex {v.shape[0]}']
    head += [f'property float {k}' for k in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
    if c is not None:
        head += ['property uchar red', 'property uchar green', 'property uchar blue']
    head += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def load_ply(path, device=None):
    """Mesh(verts, faces, normals, colors) of a PLY file that save_ply wrote -- that layout only: binary little-endian, float x y z
    nx ny nz, optionally uchar red green blue, triangles as `uchar int` lists.  The round trip is bit-exact.  device=None: numpy
    arrays (fp32 [V, 3], int32 [F, 3], fp32 [V, 3], uint8 [V, 3] or None); otherwise tensors on `device`.  ValueError for any
    other header, a face that is not a triangle, or a file of the wrong length."""
    with open(path, 'rb') as fh:
        blob = fh.read()
    end = blob.find(b'end_header\n')
    if end < 0:
        raise ValueError(f'load_ply: {path}: no PLY header')
    head = blob[:end].decode('ascii', 'replace').split('\n')
    body = blob[end + len(b'end_header\n'):]
    lines = [ln for ln in head if ln and not ln.startswith('comment')]
    props = [f'property float {k}' for k in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
    rgb = ['property uchar red', 'property uchar green', 'property uchar blue']
    try:
        if lines[:2] != ['ply', 'format binary_little_endian 1.0'] or not lines[2].startswith('element vertex '):
            raise ValueError
        V = int(lines[2].split()[2])
        colored = lines[3 + len(props):3 + len(props) + 3] == rgb
        rest = lines[3 + len(props) + (3 if colored else 0):]
        if lines[3:3 + len(props)] != props or len(rest) != 2 or not rest[0].startswith('element face ') \
                or rest[1] != 'property list uchar int vertex_indices':
            raise ValueError
        F = int(rest[0].split()[2])
    except (ValueError, IndexError):
        raise ValueError(f'load_ply: {path}: not the header save_ply writes') from None
    vfields = [(k, '<f4') for k in ('x', 'y', 'z', 'nx', 'ny', 'nz')] + ([(k, 'u1') for k in ('red', 'green', 'blue')] if colored else [])
    vdt, fdt = np.dtype(vfields), np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
    if V < 0 or F < 0 or len(body) != V * vdt.itemsize + F * fdt.itemsize:
        raise ValueError(f'load_ply: {path}: {len(body)} bytes for {V} vertices and {F} triangles')
    vert = np.frombuffer(body, vdt, V)
    face = np.frombuffer(body, fdt, F, offset=V * vdt.itemsize)
    if F and not np.all(face['n'] == 3):
        raise ValueError(f'load_ply: {path}: a face that is not a triangle')
    out = [np.stack([vert['x'], vert['y'], vert['z']], -1).astype(np.float32), np.ascontiguousarray(face['v'], np.int32).reshape(F, 3),
           np.stack([vert['nx'], vert['ny'], vert['nz']], -1).astype(np.float32),
           np.stack([vert['red'], vert['green'], vert['blue']], -1).astype(np.uint8) if colored else None]
    if device is not None:
        out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in out]
    return Mesh(*out)


def _host(a, dtype):
    return None if a is None else np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype)


def save_obj(path, mesh, texture=None):
    """Wavefront OBJ of `mesh` (tensors or numpy arrays): `v` and `vn` per vertex and `f` with 1-based indices.  With a Texture
    (bake_texture) three files: path, <stem>.mtl next to it with `map_Kd <stem>.png`, and <stem>.png (run._write_png; PNG row 0 is
    the texture's row 0, the flip of v is in texture.uv); one `vt` per face corner and faces `f a/t/n`.  Without a texture only
    path is written, faces `f a//n`.  Returns the list of the files written."""
    v, nrm, f = _host(mesh.verts, np.float64), _host(mesh.normals, np.float64), _host(mesh.faces, np.int64)
    root, _ = os.path.splitext(path)
    stem = os.path.basename(root)
    lines = ['# mvip_nerf_amd.mesh']
    files = [path]
    if texture is not None:
        from . import run
        uv = _host(texture.uv, np.float64)
        if uv.shape != (f.shape[0], 3, 2):
            raise ValueError(f'save_obj: texture.uv {uv.shape} for {f.shape[0]} faces')
        run._write_png(root + '.png', _host(texture.image, np.uint8))
        with open(root + '.mtl', 'w') as fh:
            fh.write(f'newmtl {stem}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {stem}.png\n')
        lines += [f'mtllib {stem}.mtl', f'usemtl {stem}']
        files += [root + '.mtl', root + '.png']
    lines += [f'v {x:.9g} {y:.9g} {z:.9g}' for x, y, z in v]
    if nrm is not None:
        lines += [f'vn {x:.9g} {y:.9g} {z:.9g}' for x, y, z in nrm]
    if texture is not None:
        lines += [f'vt {a:.9g} {b:.9g}' for a, b in uv.reshape(-1, 2)]
    for k, (a, b, c) in enumerate(f + 1):
        if texture is not None:
            t = 3 * k + 1
            lines.append(f'f {a}/{t}/{a} {b}/{t + 1}/{b} {c}/{t + 2}/{c}' if nrm is not None else f'f {a}/{t} {b}/{t + 1} {c}/{t + 2}')
        else:
            lines.append(f'f {a}//{a} {b}//{b} {c}//{c}' if nrm is not None else f'f {a} {b} {c}')
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return files
