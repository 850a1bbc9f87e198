"""Writes neddf_amd/csrc/mc_tables.h: the 256-case marching-cubes tables of csrc/mesh_kernels.hip.

`python tools/gen_mc_tables.py` regenerates the header; tests/test_mesh_host.py holds the committed header to this output.

Numbering (Lorensen & Cline 1987 as tabulated by Bourke, "Polygonising a scalar field"): corner c sits at
CORNERS[c] of the unit cell, edge e joins EDGES[e]; bit c of a case index is set when corner c is inside (value < iso).
The edge table (the crossed edges of a case) is the standard one.  The triangles are built here rather than copied:
on every face of the cell the crossing points are joined so that the face's inside corners are cut off one by one
(an ambiguous face -- two inside corners on a diagonal -- separates them), the segments are chained into loops and each
loop is triangulated (a fan where possible) without an inner diagonal between two points of one face.  The face rule depends on the face's four corners only, so two cells sharing a face
draw the same segments there, in opposite directions: the mesh is closed and consistently oriented.  A segment runs from
the point where a counter-clockwise walk round the face (seen from outside the cell) enters the inside to the point
where it leaves again, which makes each triangle's normal (p1 - p0) x (p2 - p0) point from the inside to the outside.
"""
import os
import sys

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
# the six faces, corners in counter-clockwise order seen from outside the cell
FACES = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]


def _edge(a, b):
    for e, (p, q) in enumerate(EDGES):
        if {p, q} == {a, b}:
            return e
    raise ValueError((a, b))


def _check_faces():
    for f in FACES:
        p = [CORNERS[c] for c in f]
        u = [p[1][i] - p[0][i] for i in range(3)]
        v = [p[2][i] - p[1][i] for i in range(3)]
        n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        centre = [sum(q[i] for q in p) / 4 - 0.5 for i in range(3)]
        assert sum(n[i] * centre[i] for i in range(3)) > 0, f        # the right-hand normal points out of the cell


def case_triangles(case):
    """Triangles of one case as edge-index triples."""
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}                                         # entry point -> exit point, one segment per pair
    for f in FACES:
        walk = [(f[i], f[(i + 1) % 4]) for i in range(4)]
        cross = [(i, inside[a]) for i, (a, b) in enumerate(walk) if inside[a] != inside[b]]
        # (i, 1): the walk leaves the inside on side i (an exit), (i, 0): it enters (an entry)
        for k, (i, leaving) in enumerate(cross):
            if leaving:
                continue
            j = cross[(k + 1) % len(cross)][0]       # the next crossing of the walk is the exit behind this entry's inside run
            nxt[_edge(*walk[i])] = _edge(*walk[j])
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        tris += _triangulate(loop)
    return tris


def _face_of(e1, e2):
    """True when the two edges lie on one face of the cell (their points on a common face)."""
    c = set(EDGES[e1]) | set(EDGES[e2])
    return any(c <= set(f) for f in FACES)


def _triangulate(loop):
    """Triangles of one loop, in loop order (which keeps the orientation): a fan from the first point that allows it, else
    any triangulation, such that no inner diagonal joins two points of one face -- on an ambiguous face the neighbouring
    cell could draw the same diagonal, and the edge would then belong to four triangles."""
    n = len(loop)

    def ok(a, b):
        return not _face_of(loop[a], loop[b])

    for s in range(n):
        if all(ok(s, (s + i) % n) for i in range(2, n - 1)):
            order = [loop[(s + i) % n] for i in range(n)]
            return [(order[0], order[i], order[i + 1]) for i in range(1, n - 1)]

    def split(ids):                     # triangulations of the sub-polygon ids (loop positions in order)
        if len(ids) < 3:
            return []
        a, b = ids[0], ids[-1]
        for k in range(1, len(ids) - 1):
            m = ids[k]
            if (k == 1 or ok(a, m)) and (k == len(ids) - 2 or ok(m, b)):
                left, right = split(ids[:k + 1]), split(ids[k:])
                if left is not None and right is not None:
                    return left + [(a, m, b)] + right
        return None

    tri = split(list(range(n)))
    assert tri is not None, loop
    return [tuple(loop[i] for i in sorted(t)) for t in tri]


def tables():
    """(edge_table[256], tri_table[256][...] as flat edge lists) with every case's crossed edges checked against its triangles."""
    _check_faces()
    edge_table, tri_table = [], []
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        mask = sum(1 << e for e, (a, b) in enumerate(EDGES) if inside[a] != inside[b])
        tris = case_triangles(case)
        assert {e for t in tris for e in t} == {e for e in range(12) if mask >> e & 1}, case
        edge_table.append(mask)
        tri_table.append([e for t in tris for e in t])
    return edge_table, tri_table


def edge_owner():
    """Per edge: offset of its lower corner in the cell and the axis it runs along, packed dx | dy << 1 | dz << 2 | axis << 3."""
    out = []
    for a, b in EDGES:
        pa, pb = CORNERS[a], CORNERS[b]
        axis = [i for i in range(3) if pa[i] != pb[i]]
        assert len(axis) == 1 and pb[axis[0]] == pa[axis[0]] + 1
        out.append(pa[0] | pa[1] << 1 | pa[2] << 2 | axis[0] << 3)
    return out


def header():
    edge_table, tri_table = tables()
    width = max(len(t) for t in tri_table) + 1
    lines = ["// mc_tables.h -- written by tools/gen_mc_tables.py (its docstring: numbering, face rule, orientation); do not edit.",
             "#pragma once", "", "namespace neddf {", "",
             "constexpr int kMcMaxTris = %d;      // triangles of the largest case" % ((width - 1) // 3), "",
             "// crossed edges of each case (bit e = edge e)",
             "__constant__ unsigned short kMcEdgeTable[256] = {"]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join("0x%03x" % m for m in edge_table[r:r + 16]) + ",")
    lines += ["};", "", "// triangles of each case: edge-index triples, -1 terminated",
              "__constant__ signed char kMcTriTable[256][%d] = {" % width]
    for t in tri_table:
        lines.append("    {" + ", ".join(str(e) for e in t + [-1] * (width - len(t))) + "},")
    lines += ["};", "",
              "// edge e belongs to the lattice point at corner EDGES[e][0] of the cell: dx | dy << 1 | dz << 2 | axis << 3",
              "__constant__ unsigned char kMcEdgeOwner[12] = {" + ", ".join(str(o) for o in edge_owner()) + "};",
              "", "}  // namespace neddf", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neddf_amd", "csrc", "mc_tables.h")
    if len(sys.argv) > 1:
        out = sys.argv[1]
    with open(out, "w") as fh:
        fh.write(header())
    print(out)
