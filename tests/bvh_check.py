"""numpy restatement of neddf_amd/csrc/bvh_kernels.hip: the sort keys, the tree (from the DEFINITION of a radix tree over the sorted keys
-- split every range at its highest differing bit -- not from Karras' per-node search, which the kernel uses), the boxes, and the
depth-first traversal with the pruning rule of include/neddf_hip.h (neddf_point_mesh_bvh_query), every fp32 operation rounded once.
The traversal is stated as "pop, test against the current best, evaluate a leaf or push both children, the nearer one on top" and run
for all queries in lockstep; it counts the leaves it evaluates.  Pairs are evaluated by pointmesh_check._pairs."""
import numpy as np

import geometry_check as gc
import pointmesh_check as pm
import raycast_check as rc

F = np.float32
D = np.float64
CELLS = (1024, 1024, 1024)
FACTOR = F(1.0 - 2.0 ** -16)
SLACK = F(2.0 ** -18)


def bounds(vertices, triangles):
    """(lo, hi) float64 [3] of the vertices of the valid triangles; a zero box without one (bvh.valid_bounds)."""
    p, ok = rc._valid_triangles(vertices, triangles)
    if not ok.any():
        return np.zeros(3), np.zeros(3)
    pv = p[ok].reshape(-1, 3)
    return pv.min(axis=0).astype(D), pv.max(axis=0).astype(D)


def _spread(x):
    x = np.asarray(x, np.int64)
    out = np.zeros_like(x)
    for b in range(10):
        out |= ((x >> b) & 1) << (3 * b)
    return out


def keys(vertices, triangles, lo, hi):
    """int64 [T]: Morton code of the cell of (min3 + max3) * 0.5 << 32 | index; 2^62 | index for an invalid triangle."""
    p, ok = rc._valid_triangles(vertices, triangles)
    j = np.arange(len(p), dtype=np.int64)
    if not len(p):
        return j
    with np.errstate(all="ignore"):
        c = ((p.min(axis=1) + p.max(axis=1)).astype(F) * F(0.5)).astype(F)
    _, cell = gc.cell_index(np.where(ok[:, None], c, F(0.0)), lo, hi, CELLS)
    code = _spread(cell[:, 0]) | (_spread(cell[:, 1]) << 1) | (_spread(cell[:, 2]) << 2)
    return np.where(ok, (code << 32) | j, (np.int64(1) << 62) | j)


def topology(sorted_keys):
    """(leaf_triangle int32 [T], children int32 [T - 1, 2], depth): node 0 is the root and covers every leaf; a node that covers the
    leaves first .. last splits behind the last key whose highest differing bit (between key first and key last) is 0; the left part
    first .. g is leaf ~g when g == first, else internal node g; the right part g + 1 .. last is leaf ~(g + 1) when g + 1 == last, else
    internal node g + 1.  depth = the most internal nodes above any leaf."""
    k = np.asarray(sorted_keys, np.int64)
    n = len(k)
    assert (np.diff(k) > 0).all()
    leaf = (k & 0x7fffffff).astype(np.int32)
    children = np.zeros((max(n - 1, 0), 2), np.int32)
    depth = 0
    todo = [(0, n - 1, 0, 1)] if n > 1 else []
    while todo:
        first, last, node, level = todo.pop()
        depth = max(depth, level)
        bit = (int(k[first]) ^ int(k[last])).bit_length() - 1
        g = first + int(np.searchsorted((k[first:last + 1] >> bit) & 1, 1)) - 1
        assert first <= g < last and node in (first, last)
        for side, (a, b) in enumerate(((first, g), (g + 1, last))):
            if a == b:
                children[node, side] = ~a
            else:
                child = b if side == 0 else a
                children[node, side] = child
                todo.append((a, b, child, level + 1))
    return leaf, children, depth


def fit_boxes(vertices, triangles, leaf, children):
    """float32 [2 T - 1, 6]: internal node i at row i, leaf k at row T - 1 + k; (+inf x 3, -inf x 3) for an invalid triangle."""
    p, ok = rc._valid_triangles(vertices, triangles)
    n = len(leaf)
    boxes = np.zeros((max(2 * n - 1, 0), 6), F)
    if not n:
        return boxes
    pl, okl = p[leaf], ok[leaf]
    boxes[n - 1:, :3] = np.where(okl[:, None], pl.min(axis=1), np.inf)
    boxes[n - 1:, 3:] = np.where(okl[:, None], pl.max(axis=1), -np.inf)
    order, todo = [], [0] if n > 1 else []
    while todo:                                                 # parents before children
        i = todo.pop()
        order.append(i)
        todo += [int(c) for c in children[i] if c >= 0]
    row = lambda c: c if c >= 0 else n - 1 + ~c
    for i in reversed(order):
        a, b = boxes[row(int(children[i, 0]))], boxes[row(int(children[i, 1]))]
        boxes[i, :3], boxes[i, 3:] = np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])
    return boxes


def build(vertices, triangles):
    """dict(lo, hi, keys, leaf, children, boxes, depth) of a mesh, as bvh.build_bvh builds it."""
    lo, hi = bounds(vertices, triangles)
    ks = np.sort(keys(vertices, triangles, lo, hi))
    leaf, children, depth = topology(ks)
    return dict(lo=lo, hi=hi, keys=ks, leaf=leaf, children=children, boxes=fit_boxes(vertices, triangles, leaf, children), depth=depth)


def _bound(box, q, s):
    """(m float32, m2 float32) of boxes [n, 6] against queries [n, 3]."""
    with np.errstate(all="ignore"):
        gap = np.maximum(np.maximum((box[:, :3] - q).astype(F), (q - box[:, 3:]).astype(F)), F(0.0)).astype(F)
        lb = np.sqrt(pm._dot(gap, gap)).astype(F)
        m = ((FACTOR * lb).astype(F) - s).astype(F)
        return m, (m * m).astype(F)


def point_mesh_bvh(queries, vertices, triangles, tree=None):
    """(d2, triangle int32, b1, b2, visits int32 [Q], max_stack): the traversal of the header for every query."""
    q = np.asarray(queries, F).reshape(-1, 3)
    tree = build(vertices, triangles) if tree is None else tree
    leaf, children, boxes = tree["leaf"], tree["children"], tree["boxes"]
    n, Q = len(leaf), len(q)
    k, ok = pm.triangle_constants(vertices, triangles)
    d2, tj, b1, b2 = np.full(Q, np.inf, F), np.full(Q, -1, np.int64), np.zeros(Q, F), np.zeros(Q, F)
    visits = np.zeros(Q, np.int32)
    fin = np.isfinite(q).all(axis=1)
    stack = np.zeros((Q, 2 * 64 + 2), np.int64)
    sp = np.zeros(Q, np.int64)
    max_stack = 0
    if n:
        with np.errstate(all="ignore"):
            s = (SLACK * np.abs(boxes[0]).max()).astype(F)
        stack[:, 0] = 0 if n > 1 else ~0
        sp[fin] = 1
        row = lambda c: np.where(c >= 0, c, n - 1 + ~c)
        while (sp > 0).any():
            max_stack = max(max_stack, int(sp.max()))
            act = np.flatnonzero(sp > 0)
            sp[act] -= 1
            node = stack[act, sp[act]]
            box = boxes[row(node)]
            m, m2 = _bound(box, q[act], s)
            skip = (box[:, 0] > box[:, 3]) | ((m > 0) & (m2 > d2[act]) & (m2 >= F(1e-30)) & (m2 < np.inf))
            act, node = act[~skip], node[~skip]
            at_leaf = node < 0
            if at_leaf.any():
                i, j = act[at_leaf], leaf[~node[at_leaf]].astype(np.int64)
                D2, c1, c2 = (x.reshape(-1) for x in pm._pairs(q[i][None], {name: x[j] for name, x in k.items()}))
                visits[i] += 1
                take = ok[j] & ((D2 < d2[i]) | ((D2 == d2[i]) & ((tj[i] < 0) | (j < tj[i]))))
                i, j = i[take], j[take]
                d2[i], tj[i], b1[i], b2[i] = D2[take], j, c1[take], c2[take]
            inner = ~at_leaf
            if inner.any():
                i, c = act[inner], children[node[inner]].astype(np.int64)
                key = []
                for side in (0, 1):
                    m, m2 = _bound(boxes[row(c[:, side])], q[i], s)
                    key.append(np.where(m > 0, m2, F(0.0)))
                swap = key[1] < key[0]                          # the left child first on a tie
                stack[i, sp[i]] = np.where(swap, c[:, 0], c[:, 1])
                stack[i, sp[i] + 1] = np.where(swap, c[:, 1], c[:, 0])
                sp[i] += 2
    d2[~fin], tj[~fin], b1[~fin], b2[~fin] = np.nan, -1, np.nan, np.nan
    return d2, tj.astype(np.int32), b1, b2, visits, max_stack
