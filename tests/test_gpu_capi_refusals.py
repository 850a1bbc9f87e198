"""The refusals of the mesh and point-geometry entry points (neddf_amd/csrc/geom_capi.hip), pinned: return code and neddf_last_error text
of every argument check that comes before the first HIP call.  Nothing is launched: pointers are NULL or one small device tensor, counts
are tiny or deliberately out of range.  The expected strings are literals -- the text a caller may already match on -- so that moving or
sharing the checks cannot change a word of them.  (The refusals behind a launch -- a capacity below a count that the device produced --
belong to the tests of their features.)"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E, U = -1, -3               # NEDDF_EINVAL, NEDDF_EUNSUPPORTED
N = None
B = 2 ** 31
T39 = 2 ** 39               # triangles whose blocks of 256 no longer fit int32
NAN, INF = math.nan, math.inf

# the arguments of every entry point after the context, in order.  A row names the ones it changes; the others take a value that passes:
# d_*: the device tensor, n_*: 1, h_n_*: a host int64, the unit box with 4 x 4 x 4 cells and the scalars below.
SIG = {
    "neddf_mesh_vertex_normals": "d_vertices n_vertices d_triangles n_triangles d_normals stream",
    "neddf_mesh_components": "d_triangles n_triangles n_vertices d_vertex_label d_triangle_label d_component_triangles h_n_components stream",
    "neddf_mesh_compact": "d_vertices n_vertices d_triangles n_triangles d_keep_triangle d_out_vertices vertex_cap d_out_triangles triangle_cap "
                          "d_vertex_map h_n_vertices h_n_triangles stream",
    "neddf_mesh_sample_count": "d_vertices n_vertices d_triangles n_triangles density seed h_n_samples stream",
    "neddf_mesh_sample_write": "d_vertices n_vertices d_triangles n_triangles density seed d_points d_triangle_id sample_cap h_n_samples stream",
    "neddf_nn_brute": "d_queries n_queries d_targets n_targets d_d2 d_index stream",
    "neddf_nn_grid_build": "d_targets n_targets h_lo h_hi h_cells d_cell_start d_order h_n_valid stream",
    "neddf_nn_grid_query": "d_queries n_queries d_targets n_targets h_lo h_hi h_cells d_cell_start d_order d_d2 d_index stream",
    "neddf_raycast_brute": "d_ray_orig d_ray_dir n_rays d_vertices n_vertices d_triangles n_triangles t_min t_max pad d_t d_triangle d_b1 d_b2 stream",
    "neddf_raycast_grid_count": "d_vertices n_vertices d_triangles n_triangles h_lo h_hi h_cells pad h_n_items stream",
    "neddf_raycast_grid_build": "d_vertices n_vertices d_triangles n_triangles h_lo h_hi h_cells pad d_cell_start d_items item_cap h_n_items stream",
    "neddf_raycast_grid_query": "d_ray_orig d_ray_dir n_rays d_vertices n_vertices d_triangles n_triangles h_lo h_hi h_cells pad d_cell_start d_items "
                                "n_items t_min t_max d_t d_triangle d_b1 d_b2 stream",
    "neddf_point_mesh_brute": "d_queries n_queries d_vertices n_vertices d_triangles n_triangles d_d2 d_triangle d_b1 d_b2 stream",
    "neddf_point_mesh_grid_query": "d_queries n_queries d_vertices n_vertices d_triangles n_triangles h_lo h_hi h_cells pad d_cell_start d_items n_items "
                                   "d_d2 d_triangle d_b1 d_b2 stream",
    "neddf_bvh_keys": "d_vertices n_vertices d_triangles n_triangles h_lo h_hi d_keys stream",
    "neddf_bvh_build": "d_vertices n_vertices d_triangles n_triangles d_sorted_keys d_leaf_triangle d_children d_boxes stream",
    "neddf_point_mesh_bvh_query": "d_queries n_queries d_vertices n_vertices d_triangles n_triangles d_leaf_triangle d_children d_boxes n_leaves d_d2 "
                                  "d_triangle d_b1 d_b2 d_visits stream",
    "neddf_mesh_simplify_keys": "d_vertices n_vertices h_lo h_hi h_cells d_keys stream",
    "neddf_mesh_simplify_clusters": "d_sorted_keys n_vertices d_vertex_cluster d_cluster_range h_n_clusters stream",
    "neddf_mesh_simplify_pairs": "d_vertices n_vertices d_triangles n_triangles d_vertex_cluster d_pairs pair_cap h_n_pairs stream",
    "neddf_mesh_simplify_place": "d_vertices n_vertices d_sorted_keys d_cluster_range n_clusters placement regularisation d_triangles n_triangles "
                                 "d_sorted_pairs n_pairs d_out stream",
    "neddf_mesh_simplify_attributes": "d_attributes n_vertices n_columns d_sorted_keys d_cluster_range n_clusters d_out stream",
    "neddf_mesh_simplify_triangles": "d_triangles n_triangles n_vertices d_vertex_cluster d_mapped d_lowest d_keys stream",
    "neddf_mesh_simplify_unique": "d_lowest d_keys n_triangles d_order d_keep_triangle stream",
}
SCALARS = {"stream": None, "density": 1.0, "seed": 0, "pad": 0.01, "t_min": 0.0, "t_max": 1.0, "vertex_cap": 1, "triangle_cap": 1, "sample_cap": 1,
           "item_cap": 1, "pair_cap": 1, "placement": 0, "regularisation": 0.0}
LO, HI, CELLS = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4)

# boxes and cells that every grid refuses the same way: (changed arguments, the refusal after the entry point's name)
BAD_BOX = [
    ({"h_lo": N}, "NULL box"), ({"h_hi": N}, "NULL box"),
    ({"h_hi": (1.0, -1.0, 1.0)}, "hi < lo"), ({"h_lo": (0.0, 0.0, NAN)}, "nan"), ({"h_hi": (NAN, 1.0, 1.0)}, "nan"), ({"h_hi": (1.0, INF, 1.0)}, "nan"),
    ({"h_lo": (-1e300, 0.0, 0.0)}, "fp32"), ({"h_hi": (1e300, 1e300, 1e300), "h_lo": (1e300, 0.0, 0.0)}, "fp32"), ({"h_hi": (1.0, 1e-300, 1.0)}, "fp32"),
]
BAD_CELLS = [({"h_cells": N}, "NULL box"), ({"h_cells": (0, 4, 4)}, "cells"), ({"h_cells": (4, 4, 1025)}, "cells"), ({"h_cells": (4, -1, 4)}, "cells")]
TOO_MANY_CELLS = {"h_cells": (512, 512, 128)}
BAD_PAD = [{"pad": -1.0}, {"pad": NAN}, {"pad": INF}, {"pad": -INF}]
SMALL_PAD = [{"pad": 1e-6}, {"pad": 0.0}, {"pad": 0.01, "h_hi": (1.0, 1000.0, 1.0)}, {"pad": 0.01, "h_lo": (-1000.0, 0.0, 0.0)}]


def pick(rows, kind):
    return [changed for changed, k in rows if k == kind]


# (entry point, return code, neddf_last_error, the argument changes that must each produce it)
TABLE = [
    ("neddf_mesh_vertex_normals", E, "mesh_vertex_normals: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_vertex_normals", E, "mesh_vertex_normals: NULL vertices, triangles or normals", [{"d_vertices": N}, {"d_triangles": N}, {"d_normals": N}]),
    ("neddf_mesh_vertex_normals", U, "mesh_vertex_normals: 2^31 vertices or more (triangle indices are int32)", [{"n_vertices": B}]),

    ("neddf_mesh_components", E, "mesh_components: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_components", E, "mesh_components: NULL triangles, vertex labels, component counts or count",
     [{"d_triangles": N}, {"d_vertex_label": N}, {"d_component_triangles": N}, {"h_n_components": N}]),
    ("neddf_mesh_components", U, "mesh_components: 2^31 vertices or more, or too many triangles", [{"n_vertices": B}, {"n_triangles": T39}]),

    ("neddf_mesh_compact", E, "mesh_compact: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_compact", E, "mesh_compact: NULL vertices, triangles, keep flags or count",
     [{"d_vertices": N}, {"d_triangles": N}, {"d_keep_triangle": N}, {"h_n_vertices": N}, {"h_n_triangles": N}]),
    ("neddf_mesh_compact", U, "mesh_compact: 2^31 vertices or more, or too many triangles", [{"n_vertices": B}, {"n_triangles": T39}]),

    ("neddf_mesh_sample_count", E, "mesh_sample: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_sample_count", E, "mesh_sample: NULL vertices, triangles or count", [{"d_vertices": N}, {"d_triangles": N}, {"h_n_samples": N}]),
    ("neddf_mesh_sample_count", E, "mesh_sample: the density must be finite and not negative", [{"density": -1.0}, {"density": NAN}, {"density": INF}]),
    ("neddf_mesh_sample_count", U, "mesh_sample: 2^31 vertices or more, or too many triangles", [{"n_vertices": B}, {"n_triangles": T39}]),
    ("neddf_mesh_sample_write", E, "mesh_sample: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_sample_write", E, "mesh_sample: NULL vertices, triangles or count", [{"d_vertices": N}, {"d_triangles": N}, {"h_n_samples": N}]),
    ("neddf_mesh_sample_write", E, "mesh_sample: the density must be finite and not negative", [{"density": -1.0}, {"density": NAN}, {"density": INF}]),
    ("neddf_mesh_sample_write", U, "mesh_sample: 2^31 vertices or more, or too many triangles", [{"n_vertices": B}, {"n_triangles": T39}]),

    ("neddf_nn_brute", E, "nn_brute: negative count", [{"n_queries": -1}, {"n_targets": -1}]),
    ("neddf_nn_brute", E, "nn_brute: NULL points", [{"d_queries": N}, {"d_targets": N}]),
    ("neddf_nn_brute", U, "nn_brute: 2^31 points or more (indices are int32)", [{"n_queries": B}, {"n_targets": B}]),
    ("neddf_nn_brute", E, "nn_brute: NULL outputs", [{"d_d2": N}, {"d_index": N}]),

    ("neddf_nn_grid_build", E, "nn_grid_build: negative count", [{"n_targets": -1}]),
    ("neddf_nn_grid_build", E, "nn_grid_build: NULL points", [{"d_targets": N}]),
    ("neddf_nn_grid_build", U, "nn_grid_build: 2^31 points or more (indices are int32)", [{"n_targets": B}]),
    ("neddf_nn_grid_build", E, "nn_grid_build: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_nn_grid_build", E, "nn_grid_build: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_nn_grid_build", E, "nn_grid_build: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_nn_grid_build", E, "nn_grid_build: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_nn_grid_build", E, "nn_grid_build: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_nn_grid_build", E, "nn_grid_build: NULL cell_start, order or count", [{"d_cell_start": N}, {"d_order": N}, {"h_n_valid": N}]),

    ("neddf_nn_grid_query", E, "nn_grid_query: negative count", [{"n_queries": -1}, {"n_targets": -1}]),
    ("neddf_nn_grid_query", E, "nn_grid_query: NULL points", [{"d_queries": N}, {"d_targets": N}]),
    ("neddf_nn_grid_query", U, "nn_grid_query: 2^31 points or more (indices are int32)", [{"n_queries": B}, {"n_targets": B}]),
    ("neddf_nn_grid_query", E, "nn_grid_query: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_nn_grid_query", E, "nn_grid_query: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_nn_grid_query", E, "nn_grid_query: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_nn_grid_query", E, "nn_grid_query: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_nn_grid_query", E, "nn_grid_query: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_nn_grid_query", E, "nn_grid_query: NULL cell_start or outputs", [{"d_cell_start": N}, {"d_d2": N}, {"d_index": N}]),

    ("neddf_raycast_brute", E, "raycast_brute: negative count", [{"n_rays": -1}, {"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_raycast_brute", E, "raycast_brute: NULL rays, vertices or triangles", [{"d_ray_orig": N}, {"d_ray_dir": N}, {"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_raycast_brute", E, "raycast_brute: pad must be finite and not negative", BAD_PAD),
    ("neddf_raycast_brute", U, "raycast_brute: 2^31 rays, triangles or vertices or more (indices are int32)", [{"n_rays": B}, {"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_raycast_brute", E, "raycast_brute: NULL outputs", [{"d_t": N}, {"d_triangle": N}, {"d_b1": N}, {"d_b2": N}]),

    ("neddf_raycast_grid_count", E, "raycast_grid_count: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: NULL rays, vertices or triangles", [{"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: pad must be finite and not negative", BAD_PAD),
    ("neddf_raycast_grid_count", U, "raycast_grid_count: 2^31 rays, triangles or vertices or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: pad below 2^-16 of the largest of |lo|, |hi| and the box extent (the grid would lose hits to rounding)",
     SMALL_PAD),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: 2 pad does not fit fp32", [{"pad": 3e38}]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: the widened box does not fit fp32",
     [{"pad": 1e37, "h_lo": (-3.3e38, 0.0, 0.0)}, {"pad": 1e37, "h_hi": (1.0, 1.0, 3.3e38)}]),
    ("neddf_raycast_grid_count", E, "raycast_grid_count: NULL count", [{"h_n_items": N}]),

    ("neddf_raycast_grid_build", E, "raycast_grid_build: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: NULL rays, vertices or triangles", [{"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: pad must be finite and not negative", BAD_PAD),
    ("neddf_raycast_grid_build", U, "raycast_grid_build: 2^31 rays, triangles or vertices or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: pad below 2^-16 of the largest of |lo|, |hi| and the box extent (the grid would lose hits to rounding)",
     SMALL_PAD),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: 2 pad does not fit fp32", [{"pad": 3e38}]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: the widened box does not fit fp32", [{"pad": 1e37, "h_lo": (-3.3e38, 0.0, 0.0)}]),
    ("neddf_raycast_grid_build", E, "raycast_grid_build: NULL cell_start or count", [{"d_cell_start": N}, {"h_n_items": N}]),

    ("neddf_raycast_grid_query", E, "raycast_grid_query: negative count", [{"n_rays": -1}, {"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: NULL rays, vertices or triangles",
     [{"d_ray_orig": N}, {"d_ray_dir": N}, {"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: pad must be finite and not negative", BAD_PAD),
    ("neddf_raycast_grid_query", U, "raycast_grid_query: 2^31 rays, triangles or vertices or more (indices are int32)",
     [{"n_rays": B}, {"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: pad below 2^-16 of the largest of |lo|, |hi| and the box extent (the grid would lose hits to rounding)",
     SMALL_PAD),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: 2 pad does not fit fp32", [{"pad": 3e38}]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: the widened box does not fit fp32", [{"pad": 1e37, "h_lo": (-3.3e38, 0.0, 0.0)}]),
    ("neddf_raycast_grid_query", E, "raycast_grid_query: NULL cell_start, items or outputs, or an item count outside [0, 2^31)",
     [{"d_cell_start": N}, {"d_items": N}, {"n_items": -1}, {"n_items": B}, {"d_t": N}, {"d_triangle": N}, {"d_b1": N}, {"d_b2": N}]),

    ("neddf_point_mesh_brute", E, "point_mesh_brute: negative count", [{"n_queries": -1}, {"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_point_mesh_brute", E, "point_mesh_brute: NULL rays, vertices or triangles", [{"d_queries": N}, {"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_point_mesh_brute", U, "point_mesh_brute: 2^31 rays, triangles or vertices or more (indices are int32)",
     [{"n_queries": B}, {"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_point_mesh_brute", E, "point_mesh_brute: NULL outputs", [{"d_d2": N}, {"d_triangle": N}, {"d_b1": N}, {"d_b2": N}]),

    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: negative count", [{"n_queries": -1}, {"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: NULL rays, vertices or triangles", [{"d_queries": N}, {"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: pad must be finite and not negative", BAD_PAD),
    ("neddf_point_mesh_grid_query", U, "point_mesh_grid_query: 2^31 rays, triangles or vertices or more (indices are int32)",
     [{"n_queries": B}, {"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: the box does not fit fp32", pick(BAD_BOX, "fp32")),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: more than 2^24 cells", [TOO_MANY_CELLS]),
    ("neddf_point_mesh_grid_query", E,
     "point_mesh_grid_query: pad below 2^-16 of the largest of |lo|, |hi| and the box extent (the grid would lose hits to rounding)", SMALL_PAD),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: 2 pad does not fit fp32", [{"pad": 3e38}]),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: the widened box does not fit fp32", [{"pad": 1e37, "h_lo": (-3.3e38, 0.0, 0.0)}]),
    ("neddf_point_mesh_grid_query", E, "point_mesh_grid_query: NULL cell_start, items or outputs, or an item count outside [0, 2^31)",
     [{"d_cell_start": N}, {"d_items": N}, {"n_items": -1}, {"n_items": B}, {"d_d2": N}, {"d_triangle": N}, {"d_b1": N}, {"d_b2": N}]),

    ("neddf_bvh_keys", E, "bvh_keys: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_bvh_keys", E, "bvh_keys: NULL rays, vertices or triangles", [{"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_bvh_keys", U, "bvh_keys: 2^31 rays, triangles or vertices or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_bvh_keys", E, "bvh_keys: NULL box", pick(BAD_BOX, "NULL box")),
    ("neddf_bvh_keys", E, "bvh_keys: NULL keys", [{"d_keys": N}]),
    ("neddf_bvh_keys", E, "bvh_keys: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_bvh_keys", E, "bvh_keys: the box does not fit fp32", pick(BAD_BOX, "fp32")),

    ("neddf_bvh_build", E, "bvh_build: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_bvh_build", E, "bvh_build: NULL rays, vertices or triangles", [{"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_bvh_build", U, "bvh_build: 2^31 rays, triangles or vertices or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_bvh_build", E, "bvh_build: NULL keys, leaf_triangle, children or boxes",
     [{"d_sorted_keys": N}, {"d_leaf_triangle": N}, {"d_boxes": N}, {"d_children": N, "n_triangles": 2}]),

    ("neddf_point_mesh_bvh_query", E, "point_mesh_bvh_query: negative count", [{"n_queries": -1}, {"n_vertices": -1}, {"n_triangles": -1, "n_leaves": -1}]),
    ("neddf_point_mesh_bvh_query", E, "point_mesh_bvh_query: NULL rays, vertices or triangles", [{"d_queries": N}, {"d_vertices": N}, {"d_triangles": N}]),
    ("neddf_point_mesh_bvh_query", U, "point_mesh_bvh_query: 2^31 rays, triangles or vertices or more (indices are int32)",
     [{"n_queries": B}, {"n_vertices": B}, {"n_triangles": B, "n_leaves": B}]),
    ("neddf_point_mesh_bvh_query", E, "point_mesh_bvh_query: the tree's leaves are not this mesh's triangles (n_leaves != n_triangles)",
     [{"n_leaves": 2}, {"n_leaves": 0}, {"n_triangles": 3}]),
    ("neddf_point_mesh_bvh_query", E, "point_mesh_bvh_query: NULL leaf_triangle, children or boxes",
     [{"d_leaf_triangle": N}, {"d_boxes": N}, {"d_children": N, "n_triangles": 2, "n_leaves": 2}]),
    ("neddf_point_mesh_bvh_query", E, "point_mesh_bvh_query: NULL outputs", [{"d_d2": N}, {"d_triangle": N}, {"d_b1": N}, {"d_b2": N}]),

    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: negative count", [{"n_vertices": -1}]),
    ("neddf_mesh_simplify_keys", U, "mesh_simplify_keys: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}]),
    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: NULL box or cells", pick(BAD_BOX + BAD_CELLS, "NULL box")),
    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: NULL vertices or keys", [{"d_vertices": N}, {"d_keys": N}]),
    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: 1 to 1024 cells per axis", pick(BAD_CELLS, "cells")),
    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: a finite box with hi >= lo expected", pick(BAD_BOX, "hi < lo") + pick(BAD_BOX, "nan")),
    ("neddf_mesh_simplify_keys", E, "mesh_simplify_keys: the box does not fit fp32", pick(BAD_BOX, "fp32")),

    ("neddf_mesh_simplify_clusters", E, "mesh_simplify_clusters: negative count", [{"n_vertices": -1}]),
    ("neddf_mesh_simplify_clusters", U, "mesh_simplify_clusters: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}]),
    ("neddf_mesh_simplify_clusters", E, "mesh_simplify_clusters: NULL keys, vertex clusters, cluster ranges or count",
     [{"d_sorted_keys": N}, {"d_vertex_cluster": N}, {"d_cluster_range": N}, {"h_n_clusters": N}]),

    ("neddf_mesh_simplify_pairs", E, "mesh_simplify_pairs: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_simplify_pairs", U, "mesh_simplify_pairs: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_mesh_simplify_pairs", E, "mesh_simplify_pairs: NULL vertices, triangles, vertex clusters or count",
     [{"d_vertices": N}, {"d_triangles": N}, {"d_vertex_cluster": N}, {"h_n_pairs": N}]),

    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_simplify_place", U, "mesh_simplify_place: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: 0 <= clusters <= vertices and 0 <= pairs <= 3 triangles expected",
     [{"n_clusters": 2}, {"n_clusters": -1}, {"n_pairs": -1}, {"n_pairs": 4}]),
    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: unknown placement", [{"placement": 2}, {"placement": -1}]),
    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: the regularisation must be finite and not negative",
     [{"regularisation": NAN}, {"regularisation": -1.0}, {"regularisation": INF}]),
    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: NULL vertices, keys, ranges or output",
     [{"d_vertices": N}, {"d_sorted_keys": N}, {"d_cluster_range": N}, {"d_out": N}]),
    ("neddf_mesh_simplify_place", E, "mesh_simplify_place: NULL triangles or pairs",
     [{"placement": 1, "n_pairs": 1, "d_triangles": N}, {"placement": 1, "n_pairs": 1, "d_sorted_pairs": N}]),

    ("neddf_mesh_simplify_attributes", E, "mesh_simplify_attributes: negative count", [{"n_vertices": -1}]),
    ("neddf_mesh_simplify_attributes", U, "mesh_simplify_attributes: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}]),
    ("neddf_mesh_simplify_attributes", E, "mesh_simplify_attributes: 0 <= clusters <= vertices and 1 to 1024 columns expected",
     [{"n_clusters": 2}, {"n_clusters": -1}, {"n_columns": 0}, {"n_columns": 1025}]),
    ("neddf_mesh_simplify_attributes", E, "mesh_simplify_attributes: NULL attributes, keys, ranges or output",
     [{"d_attributes": N}, {"d_sorted_keys": N}, {"d_cluster_range": N}, {"d_out": N}]),

    ("neddf_mesh_simplify_triangles", E, "mesh_simplify_triangles: negative count", [{"n_vertices": -1}, {"n_triangles": -1}]),
    ("neddf_mesh_simplify_triangles", U, "mesh_simplify_triangles: 2^31 vertices or triangles or more (indices are int32)", [{"n_vertices": B}, {"n_triangles": B}]),
    ("neddf_mesh_simplify_triangles", E, "mesh_simplify_triangles: NULL triangles, vertex clusters or outputs",
     [{"d_triangles": N}, {"d_vertex_cluster": N}, {"d_mapped": N}, {"d_lowest": N}, {"d_keys": N}]),

    ("neddf_mesh_simplify_unique", E, "mesh_simplify_unique: negative count", [{"n_triangles": -1}]),
    ("neddf_mesh_simplify_unique", U, "mesh_simplify_unique: 2^31 vertices or triangles or more (indices are int32)", [{"n_triangles": B}]),
    ("neddf_mesh_simplify_unique", E, "mesh_simplify_unique: NULL triples, order or keep flags",
     [{"d_lowest": N}, {"d_keys": N}, {"d_order": N}, {"d_keep_triangle": N}]),
]


@pytest.fixture(scope="module")
def capi():
    from neddf_amd import _lib
    ctx = _lib.Context.get("cuda:0")
    keep = {"tensor": torch.zeros(16, dtype=torch.float32, device=ctx.device)}

    def call(name, changed):
        """(return code, neddf_last_error) of one call; the message of an unrelated refusal is planted first, so a stale one cannot pass"""
        unknown = set(changed) - set(SIG[name].split())
        assert not unknown, (name, unknown)
        args = []
        for p in SIG[name].split():
            v = changed[p] if p in changed else SCALARS[p] if p in SCALARS else {"h_lo": LO, "h_hi": HI, "h_cells": CELLS}.get(p, p)
            if v == p:                  # the default of its kind
                v = 1 if p.startswith("n_") else C.byref(_lib._i64(0)) if p.startswith("h_n_") else C.c_void_p(keep["tensor"].data_ptr())
            elif isinstance(v, tuple):
                v = (C.c_int * 3)(*v) if p == "h_cells" else (C.c_double * 3)(*v)
            args.append(v)
        assert ctx.lib.neddf_mesh_simplify_unique(ctx.h, None, None, -1, None, None, None) == E
        assert ctx.lib.neddf_last_error(ctx.h) == b"mesh_simplify_unique: negative count"
        rc = getattr(ctx.lib, name)(ctx.h, *args)
        return rc, ctx.lib.neddf_last_error(ctx.h).decode()

    return call


@pytest.mark.parametrize("name", list(SIG))
def test_refusals_keep_their_code_and_text(capi, name):
    rows = [r for r in TABLE if r[0] == name]
    assert rows
    for _, code, text, changes in rows:
        assert changes, text
        for changed in changes:
            assert capi(name, changed) == (code, text), (name, changed)


def test_every_entry_point_answers_a_null_context_without_touching_its_arguments():
    from neddf_amd import _lib
    lib = _lib.load()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in list(SIG) + ["neddf_mesh_components_rounds"]:
        call = [a(0) if a in (C.c_int, C.c_int64) else a(0.0) if a in (C.c_float, C.c_double) else None for a in bound[name]]
        assert getattr(lib, name)(*call) == E, name


def test_simplify_keys_takes_more_cells_than_the_lists_do(capi):
    """2^25 cells: the 2^24 limit is the cell lists', not the cell function's.  With no vertex nothing is launched and the call succeeds."""
    assert capi("neddf_mesh_simplify_keys", dict(TOO_MANY_CELLS, n_vertices=0, d_vertices=N, d_keys=N))[0] == 0
    assert capi("neddf_mesh_simplify_keys", {"h_cells": (1024, 1024, 1024), "n_vertices": 0})[0] == 0


def test_bvh_keys_never_speaks_of_cells(capi):
    """neddf_bvh_keys has no cells argument: whatever it refuses, it does not say `cells per axis`."""
    assert capi("neddf_bvh_keys", {"h_lo": (0.0, NAN, 0.0)}) == (E, "bvh_keys: a finite box with hi >= lo expected")
    seen = 0
    for name, _, _, changes in TABLE:
        for changed in changes if name == "neddf_bvh_keys" else []:
            rc, text = capi(name, changed)
            assert rc != 0 and "cells" not in text, (changed, text)
            seen += 1
    assert seen >= 12
    assert capi("neddf_bvh_keys", {"n_triangles": 0, "d_triangles": N, "d_keys": N})[0] == 0            # and a degenerate box is no refusal
    assert capi("neddf_bvh_keys", {"n_triangles": 0, "h_hi": LO})[0] == 0
