"""`python neddf/scripts/extract_mesh.py <run_dir> [--epoch 2000] [--resolution 64] [--threshold 0.0275] [--field distance]
[--cube-range 1.1] [--normals [field|geometric]] [--colors] [--min-component N] [--keep-largest [K]] [--sparse [B]] [--band W]
[--lipschitz L] [--brick-dilate D] [--simplify [K]] [--simplify-placement mean|quadric] [--check-distance [BAND]] [--check-volume [N]]` -- the reference's mesh export (neddf/scripts/fields_visualizer.py:528-566, generate_mesh: voxelize
"distance" on a 64^3 cube of half-width 1.1, marching cubes at 0.0275, export) without its Open3D viewer.  The run is
loaded as run_eval loads it (`<run_dir>/.hydra/config.yaml`, `models/model_{epoch:05}.pth`); the mesh of
`trainer.neural_render.get_network()` is written to `<run_dir>/mesh/mesh_{resolution}_threshold{threshold}.ply` (the
reference's file name, PLY in place of collada), in world coordinates.  Prints the vertex and triangle counts and the wall
time of the grid evaluation and of marching cubes.  --normals adds per-vertex normals (`property float nx, ny, nz`): the field's
own (NeDDF, NeuS; the default where the field has one) or geometric ones; --colors adds the colour trunk's value at every vertex
seen straight on (`property uchar red, green, blue`).  Without them the file is the plain positions-and-triangles PLY.
--min-component N drops the connected components with fewer than N triangles and --keep-largest [K] all but the K (default 1)
largest, on the device and before normals and colours; one more line then reports the components found and kept, the triangles
removed and the clean-up time.
--sparse [B] (B = 8 when omitted) evaluates the field only on the bricks of B^3 cells that can hold the level set, picked from the
field's values at the brick corners: a corner within --band of the threshold keeps a brick (default: --lipschitz, 1 when omitted,
times half the brick's diagonal; a density needs an explicit --band), --brick-dilate grows the set.  The mesh and the file are the
dense run's whenever no brick the surface crosses was left out; one more line reports the active and the total number of bricks.
--check-distance [BAND] (distance and sdf fields) measures the field against the mesh just extracted (BaseNeuralField.level_set_check:
|D(p) - threshold| against the exact distance from p to the mesh at points within BAND of it; BAND = four lattice steps of this run's
resolution when omitted) and prints the result as ONE JSON line after everything else.  Without the option nothing new runs.
--check-volume [N] (distance and sdf fields) is its whole-volume counterpart (BaseNeuralField.distance_field_check: N points, 100 000
when omitted, spread over the mesh's bounds widened by a quarter of their diagonal; the error and the slope by distance from the
surface, through the triangles' BVH) and prints ONE more JSON line, after --check-distance's.
--simplify [K] (K = 2 when omitted) merges the vertices of every cell of K lattice steps, K * 2 cube_range / (resolution - 1), into one
(mesh.simplify_mesh: the cell's mean, or with --simplify-placement quadric the point closest to the planes of the triangles around it),
after the clean-up and before normals and colours; one more line reports the vertex and triangle counts before and after and the
time.  With --check-distance or --check-volume the unsimplified mesh is extracted as well and one further line gives the largest
distance from the simplified surface to it (geometry.mesh_distance, to="surface"); both checks then measure the simplified mesh."""
import json
from argparse import ArgumentParser
from pathlib import Path

from neddf_amd.mesh import write_ply
from neddf_amd.scripts.run_eval import load_config, load_trainer


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument("output_dir", type=Path, help="directory path where models are located")
    parser.add_argument("--epoch", type=int, default=2000, help="epoch number of model")
    parser.add_argument("--resolution", type=int, default=64, help="lattice points per axis")
    parser.add_argument("--threshold", type=float, default=0.0275, help="iso-level of the field")
    parser.add_argument("--field", default="distance", help="distance (NeDDF), sdf (NeuS) or density")
    parser.add_argument("--cube-range", type=float, default=1.1, help="half-width of the meshed cube")
    parser.add_argument("--normals", nargs="?", const="auto", default=None, choices=["auto", "field", "geometric"],
                        help="write vertex normals: the field's own (default for NeDDF / NeuS) or geometric ones (NeRF)")
    parser.add_argument("--colors", action="store_true", help="write vertex colours (the colour trunk seen against the normal)")
    parser.add_argument("--min-component", type=int, default=0, metavar="N", help="drop connected components with fewer than N triangles")
    parser.add_argument("--keep-largest", type=int, nargs="?", const=1, default=0, metavar="K",
                        help="keep only the K largest connected components (K = 1 when omitted)")
    parser.add_argument("--sparse", type=int, nargs="?", const=8, default=0, metavar="B",
                        help="sparse extraction in bricks of B^3 cells, 2..16 (B = 8 when omitted)")
    parser.add_argument("--band", type=float, default=None, help="a brick corner this close to the threshold keeps its brick")
    parser.add_argument("--lipschitz", type=float, default=1.0, help="the default band is this times half the brick's diagonal")
    parser.add_argument("--brick-dilate", type=int, default=0, metavar="D", help="grow the set of kept bricks by D bricks (0..4)")
    parser.add_argument("--simplify", type=float, nargs="?", const=2.0, default=0.0, metavar="K",
                        help="vertex clustering in cells of K lattice steps (K = 2 when omitted)")
    parser.add_argument("--simplify-placement", default="mean", choices=["mean", "quadric"],
                        help="the merged vertex: the cell's mean, or the point closest to the planes of the triangles around it")
    parser.add_argument("--check-distance", type=float, nargs="?", const=0.0, default=None, metavar="BAND",
                        help="check the field against the exact distance to the extracted mesh within BAND of it (four lattice steps when omitted)")
    parser.add_argument("--check-volume", type=int, nargs="?", const=100000, default=None, metavar="N",
                        help="check the field against the exact distance to the extracted mesh at N points of the whole volume (100000 when omitted)")
    return parser


def main(argv=None) -> Path:
    args = build_parser().parse_args(argv)
    output_dir = args.output_dir.resolve()
    trainer = load_trainer(load_config(output_dir), output_dir, args.epoch)
    trainer.neural_render.set_iter(-1)                  # the evaluation state, as render_all sets it
    network = trainer.neural_render.get_network()
    times = {}
    normals, colors = None, None
    clean = {}
    if args.min_component or args.keep_largest:
        clean = dict(min_component_triangles=args.min_component, keep_largest=args.keep_largest)
    if args.sparse:
        clean = dict(clean, brick=args.sparse, band=args.band, lipschitz=args.lipschitz, brick_dilate=args.brick_dilate)
    if args.simplify < 0.0:
        raise SystemExit("--simplify needs a positive number of lattice steps")
    if args.simplify:
        plain = dict(clean)
        clean = dict(clean, simplify_cell=args.simplify * 2.0 * args.cube_range / max(args.resolution - 1, 1), simplify_placement=args.simplify_placement)
    if args.normals or args.colors:
        want_n = True if args.normals == "auto" else (args.normals or False)
        res = list(network.extract_mesh(args.field, args.threshold, args.cube_range, args.resolution, timings=times,
                                        normals=want_n, colors=args.colors, **clean))
        verts, tris = res[0], res[1]
        normals = res[2] if want_n else None
        colors = res[-1] if args.colors else None
    else:
        verts, tris = network.extract_mesh(args.field, args.threshold, args.cube_range, args.resolution, timings=times, **clean)
    save_dir = output_dir / "mesh"
    save_dir.mkdir(exist_ok=True)
    path = save_dir / "mesh_{}_threshold{}.ply".format(args.resolution, args.threshold)
    if normals is None and colors is None:
        write_ply(path, verts, tris)
    else:
        write_ply(path, verts, tris, normals=normals, colors=colors)
    print("vertices: %d, triangles: %d" % (verts.shape[0], tris.shape[0]))
    print("grid evaluation: %.3f s, marching cubes: %.3f s" % (times["grid"], times["mcubes"]))
    if args.sparse:
        print("bricks: %d active of %d, corner evaluation and selection: %.3f s" % (times["bricks_active"], times["bricks"], times["coarse"]))
    if "clean" in times:
        print("components: %d found, %d kept, triangles removed: %d, clean-up: %.3f s"
              % (times["components"], times["components_kept"], times["triangles_removed"], times["clean"]))
    if "simplify" in times:
        print("simplified (%s, cells of %g lattice steps): %d -> %d vertices, %d -> %d triangles, %.3f s"
              % (args.simplify_placement, args.simplify, times["vertices_before"], verts.shape[0], times["triangles_before"], tris.shape[0],
                 times["simplify"]))
    print("wrote %s" % path)
    if args.simplify and (args.check_distance is not None or args.check_volume is not None):
        from neddf_amd.geometry import mesh_distance
        full = network.extract_mesh(args.field, args.threshold, args.cube_range, args.resolution, **plain)
        if tris.shape[0] and full[1].shape[0]:
            d = mesh_distance((verts, tris), full, n=100000, to="surface", method="bvh")
            print("simplified -> unsimplified surface: max %.6g, mean %.6g over %d samples" % (d["a_to_b_max"], d["a_to_b_mean"], d["n_a"]))
        else:
            print("simplified -> unsimplified surface: no triangles to measure")
    if args.check_distance is not None:
        if args.field == "density":
            raise SystemExit("--check-distance needs a distance or sdf field")
        band = args.check_distance if args.check_distance > 0.0 else 4.0 * 2.0 * args.cube_range / max(args.resolution - 1, 1)
        print(json.dumps(network.level_set_check(verts, tris, threshold=args.threshold, band=band)))
    if args.check_volume is not None:
        if args.field == "density":
            raise SystemExit("--check-volume needs a distance or sdf field")
        print(json.dumps(network.distance_field_check(verts, tris, threshold=args.threshold, n=args.check_volume)))
    return path


if __name__ == "__main__":
    main()
