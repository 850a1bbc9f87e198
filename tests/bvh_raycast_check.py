"""numpy restatement of the ray traversal of neddf_amd/csrc/bvh_kernels.hip (rc_bvh_kernel) by the rule of include/neddf_hip.h
(neddf_raycast_bvh_query): the tree is bvh_check.build's, the box test is fp64 with every operation rounded once, and the traversal is
stated as "pop, test against the current best, evaluate a leaf or push both children, the nearer one on top" and run for all rays in
lockstep; it counts the leaves it evaluates.  Pairs are evaluated by raycast_check.cast_rays on single triangles."""
import numpy as np

import bvh_check as bc
import raycast_check as rc

F = np.float32
D = np.float64


def _ray_ok(o, d):
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)


def walks(origins, tree, pad):
    """bool [R]: the rays that walk the tree (the others visit every valid triangle in index order)."""
    o = np.asarray(origins, F).reshape(-1, 3)
    if not len(tree["boxes"]):
        return np.zeros(len(o), bool)
    with np.errstate(all="ignore"):
        w = D(np.fmax.reduce(np.abs(tree["boxes"][0]), initial=F(0.0)))
        pd = D(F(pad))
        far = D(2.0 ** 21) * pd - D(2.0) * (w + D(2.0) * pd)
        return (F(pad) >= F(2.0 ** -126)) & (pd >= D(2.0 ** -16) * w) & (np.abs(o).max(axis=1).astype(D) <= far)


def _pair(o, d, vertices, triangles, j, t_min, t_max, pad):
    """Ray i against triangle j[i] alone: (candidate bool, t, b1, b2)."""
    n = len(j)
    cand, t, b1, b2 = np.zeros(n, bool), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    for jj in np.unique(j):
        m = np.flatnonzero(j == jj)
        tt, hit, c1, c2 = rc.cast_rays(o[m], d[m], vertices, tri[jj:jj + 1], t_min=t_min, t_max=t_max, pad=pad)
        cand[m], t[m], b1[m], b2[m] = hit >= 0, tt, c1, c2
    return cand, t, b1, b2


def _take(i, j, pair, best):
    """The tie rule: best = (t, triangle, b1, b2) of all rays, updated at rays i by their pairs with triangles j."""
    cand, t, c1, c2 = pair
    bt, bj, b1, b2 = best
    take = cand & ((t < bt[i]) | ((t == bt[i]) & ((bj[i] < 0) | (j < bj[i]))))
    i, j = i[take], j[take]
    bt[i], bj[i], b1[i], b2[i] = t[take], j, c1[take], c2[take]


def _box(boxes, row, o, rcp, zero, t0, t1, pad2):
    """(te, skip-for-geometry bool) of box rows [n] against rays (o, rcp, zero [n, 3]): all fp64, one rounded operation each."""
    with np.errstate(all="ignore"):
        b = boxes[row].astype(D)
        wl, wh = b[:, :3] - pad2, b[:, 3:] + pad2
        ta, tb = (wl - o) * rcp, (wh - o) * rcp
        near = np.where(zero, -np.inf, np.fmin(ta, tb))
        far = np.where(zero, np.inf, np.fmax(ta, tb))
        te = np.fmax(t0, np.fmax.reduce(near, axis=1))
        tx = np.fmin(t1, np.fmin.reduce(far, axis=1))
        out = (zero & ((o < wl) | (o > wh))).any(axis=1)
        return te, (boxes[row, 0] > boxes[row, 3]) | out | ~(te <= tx)


def cast_rays_bvh(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, pad=0.0, tree=None, any_hit=False):
    """(t, triangle int32, b1, b2, visits int32 [R], max_stack): the traversal of the header for every ray -- the fallback for the rays
    that do not walk.  any_hit: every ray stops at its first candidate (triangle >= 0 is then the occlusion flag)."""
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(dirs, F).reshape(-1, 3)
    tree = bc.build(vertices, triangles) if tree is None else tree
    leaf, children, boxes = tree["leaf"], tree["children"], tree["boxes"]
    n, R = len(leaf), len(o)
    _, valid = rc._valid_triangles(vertices, triangles)
    best = (np.full(R, np.inf, F), np.full(R, -1, np.int64), np.zeros(R, F), np.zeros(R, F))
    visits = np.zeros(R, np.int32)
    ok = _ray_ok(o, d)
    walk = walks(o, tree, pad) & ok
    args = (vertices, triangles)
    # ---- the rays that do not walk: every valid triangle in index order
    flat = np.flatnonzero(ok & ~walk)
    if len(flat) and n:
        for j in np.flatnonzero(valid):
            i = flat[best[1][flat] < 0] if any_hit else flat
            if not len(i):
                break
            jj = np.full(len(i), j, np.int64)
            _take(i, jj, _pair(o[i], d[i], *args, jj, t_min, t_max, pad), best)
            visits[i] += 1
    # ---- the walk
    max_stack = 0
    if n and walk.any():
        with np.errstate(all="ignore"):
            zero = d == 0
            rcp = np.where(zero, D(0.0), D(1.0) / np.where(zero, F(1.0), d).astype(D))
        o64, t0, t1, pad2 = o.astype(D), D(F(t_min)), D(F(t_max)), D(2.0) * D(F(pad))
        stack = np.zeros((R, 2 * 64 + 2), np.int64)
        sp = np.zeros(R, np.int64)
        stack[:, 0] = 0 if n > 1 else ~0
        sp[walk] = 1
        row = lambda c: np.where(c >= 0, c, n - 1 + ~c)
        while (sp > 0).any():
            max_stack = max(max_stack, int(sp.max()))
            act = np.flatnonzero(sp > 0)
            sp[act] -= 1
            node = stack[act, sp[act]]
            te, skip = _box(boxes, row(node), o64[act], rcp[act], zero[act], t0, t1, pad2)
            skip |= te > best[0][act].astype(D)
            act, node = act[~skip], node[~skip]
            at_leaf = node < 0
            if at_leaf.any():
                i, j = act[at_leaf], leaf[~node[at_leaf]].astype(np.int64)
                i, j = i[valid[j]], j[valid[j]]
                _take(i, j, _pair(o[i], d[i], *args, j, t_min, t_max, pad), best)
                visits[i] += 1
                if any_hit:
                    sp[i[best[1][i] >= 0]] = 0
            inner = ~at_leaf
            if inner.any():
                i, c = act[inner], children[node[inner]].astype(np.int64)
                key = [_box(boxes, row(c[:, side]), o64[i], rcp[i], zero[i], t0, t1, pad2)[0] for side in (0, 1)]
                swap = key[1] < key[0]                          # the left child first on a tie
                stack[i, sp[i]] = np.where(swap, c[:, 0], c[:, 1])
                stack[i, sp[i] + 1] = np.where(swap, c[:, 1], c[:, 0])
                sp[i] += 2
    bt, bj, b1, b2 = best
    bt[~ok], bj[~ok], b1[~ok], b2[~ok] = np.nan, -1, np.nan, np.nan
    return bt, bj.astype(np.int32), b1, b2, visits, max_stack


def occluded_bvh(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, pad=0.0, tree=None):
    """(occluded bool [R], visits int32 [R]): the any-hit variant."""
    out = cast_rays_bvh(origins, dirs, vertices, triangles, t_min, t_max, pad, tree, any_hit=True)
    return out[1] >= 0, out[4]


def fallback(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, pad=0.0):
    """(t, triangle, b1, b2, visits): what a ray that does not walk gets -- every valid triangle, the brute restatement's bits."""
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(dirs, F).reshape(-1, 3)
    _, valid = rc._valid_triangles(vertices, triangles)
    visits = np.where(_ray_ok(o, d), valid.sum(), 0).astype(np.int32)
    return rc.cast_rays(o, d, vertices, triangles, t_min=t_min, t_max=t_max, pad=pad) + (visits,)
