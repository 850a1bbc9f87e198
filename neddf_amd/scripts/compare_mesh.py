"""`python neddf/scripts/compare_mesh.py A.ply B.ply [--samples N | --density D] [--seed S] [--tau T] [--method grid|brute|bvh] [--exact]` -- the
distance between two triangle meshes (no reference counterpart: its evaluation compares images): both are read (neddf_amd.mesh.read_ply:
the files extract_mesh.py writes, or ASCII PLY), uploaded, sampled on the device with one density and seed, and compared by
neddf_amd.geometry.mesh_distance.  Prints ONE JSON line: a_to_b_mean, b_to_a_mean, chamfer, hausdorff, a_to_b_max, b_to_a_max, n_a, n_b,
invalid_a, invalid_b, density, with --tau also precision, recall and fscore, plus the arguments and the two files.  --samples N
(default 100 000) asks for about N points per mesh; --density D for D points per unit area instead.  --exact measures every sample
against the other mesh's TRIANGLES (mesh_distance(to="surface")) instead of against its samples: no sampling floor, the mode for two
meshes that differ slightly; the line then carries "to": "surface"."""
import json
from argparse import ArgumentParser
from pathlib import Path


def build_parser() -> ArgumentParser:
    parser = ArgumentParser()
    parser.add_argument("mesh_a", type=Path, help="PLY file of the first mesh")
    parser.add_argument("mesh_b", type=Path, help="PLY file of the second mesh")
    how = parser.add_mutually_exclusive_group()
    how.add_argument("--samples", type=int, default=None, metavar="N", help="about N surface samples per mesh (default 100000)")
    how.add_argument("--density", type=float, default=None, metavar="D", help="D surface samples per unit area")
    parser.add_argument("--seed", type=int, default=0, help="seed of the sampling (32 bits)")
    parser.add_argument("--tau", type=float, default=None, help="distance threshold of precision / recall / F-score")
    parser.add_argument("--method", default="grid", choices=["grid", "brute", "bvh"],
                        help="nearest-neighbour search; bvh (with --exact only): the triangles' bounding-volume hierarchy")
    parser.add_argument("--exact", action="store_true", help="measure samples against the other mesh's triangles, not its samples")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.samples is None and args.density is None:
        args.samples = 100000
    if args.samples is not None and args.samples < 1:
        parser.error("--samples must be positive")
    if args.density is not None and not args.density > 0.0:
        parser.error("--density must be positive")
    if args.tau is not None and not args.tau >= 0.0:
        parser.error("--tau must not be negative")
    if not 0 <= args.seed < 2 ** 32:
        parser.error("--seed must fit 32 bits")
    if args.method == "bvh" and not args.exact:
        parser.error("--method bvh searches triangles: it needs --exact")
    return args


def main(argv=None) -> dict:
    args = parse_args(argv)
    import torch

    from neddf_amd.geometry import mesh_distance
    from neddf_amd.mesh import read_ply
    dev = torch.device("cuda:0")
    meshes = [tuple(torch.from_numpy(a).to(dev) for a in read_ply(p)) for p in (args.mesh_a, args.mesh_b)]
    out = mesh_distance(meshes[0], meshes[1], n=args.samples, density=args.density, seed=args.seed, tau=args.tau, method=args.method,
                        to="surface" if args.exact else "samples")
    out.update(mesh_a=str(args.mesh_a), mesh_b=str(args.mesh_b), seed=args.seed, method=args.method, tau=args.tau)
    if args.exact:
        out["to"] = "surface"
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
