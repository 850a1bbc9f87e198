"""numpy float32 restatement of the sphere-tracing kernels (include/neddf_hip.h "sphere tracing"; neddf_amd/csrc/trace_kernels.hip),
operation by operation: every product, sum and difference is one float32 numpy operation, i.e. one rounding, in the order the header
states.  The distances are an INPUT of every step (the caller evaluates them at the points the restatement -- or the GPU -- hands
out), so the restatement says nothing about a field: it pins begin / compact / advance / bisect / finish, bit for bit."""
import numpy as np

ACTIVE, HIT, MISS, EXHAUSTED, INVALID = 0, 1, 2, 3, 4
F = np.float32


def begin(origins, dirs, t_near):
    """State dict: t = t_lo = t_near, steps = 0, distance = NaN, status ACTIVE or (a non-finite origin / direction component) INVALID."""
    o, d = np.asarray(origins, F), np.asarray(dirs, F)
    n = o.shape[0]
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    return dict(t=np.full(n, t_near, F), t_lo=np.full(n, t_near, F), status=np.where(ok, ACTIVE, INVALID).astype(np.uint8),
                steps=np.zeros(n, np.int32), distance=np.full(n, np.nan, F))


def _points(origins, dirs, index, depth):
    o, d = np.asarray(origins, F)[index], np.asarray(dirs, F)[index]
    with np.errstate(all="ignore"):
        return (o + (depth[:, None] * d).astype(F)).astype(F)          # the rounded product, then the rounded sum


def compact(origins, dirs, st):
    """(index int32 [M] ascending, pos float32 [M, 3]) of the ACTIVE rays: pos = o + t * d."""
    index = np.flatnonzero(st["status"] == ACTIVE).astype(np.int32)
    return index, _points(origins, dirs, index, st["t"][index])


def advance(st, index, D, threshold, step_scale, min_step, t_far):
    """One step of the rays index[k] from the distances D[k]; st changes in place."""
    threshold, step_scale, min_step, t_far = F(threshold), F(step_scale), F(min_step), F(t_far)
    D = np.asarray(D, F)
    r = np.asarray(index, np.int64)
    st["distance"][r] = D
    nan = np.isnan(D)
    with np.errstate(all="ignore"):
        hit = ~nan & (D <= threshold)
        go = ~nan & ~hit
        st["status"][r[nan]] = INVALID
        st["status"][r[hit]] = HIT
        g = r[go]
        t0 = st["t"][g]
        step = np.maximum((step_scale * (D[go] - threshold).astype(F)).astype(F), min_step)
        t1 = (t0 + step).astype(F)
        st["t_lo"][g] = t0
        st["t"][g] = t1
        st["steps"][g] += 1
        st["status"][g[~(t1 <= t_far)]] = MISS


def finish(st):
    """ACTIVE -> EXHAUSTED."""
    st["status"][st["status"] == ACTIVE] = EXHAUSTED


def _mid(st, r):
    with np.errstate(all="ignore"):
        return (F(0.5) * (st["t_lo"][r] + st["t"][r]).astype(F)).astype(F)


def bisect_points(origins, dirs, st):
    """(index, pos) of the HIT rays with t_lo < t at mid = 0.5 * (t_lo + t)."""
    with np.errstate(all="ignore"):
        index = np.flatnonzero((st["status"] == HIT) & (st["t_lo"] < st["t"])).astype(np.int32)
    return index, _points(origins, dirs, index, _mid(st, index))


def bisect_update(st, index, D, threshold):
    """D <= threshold or NaN: t = mid, distance = D; otherwise t_lo = mid."""
    D = np.asarray(D, F)
    r = np.asarray(index, np.int64)
    mid = _mid(st, r)
    with np.errstate(all="ignore"):
        inside = np.isnan(D) | (D <= F(threshold))
    st["t"][r[inside]] = mid[inside]
    st["distance"][r[inside]] = D[inside]
    st["t_lo"][r[~inside]] = mid[~inside]


def trace(origins, dirs, distance_fn, threshold, t_near, t_far, max_steps, step_scale, min_step, refine):
    """The whole loop (neddf_trace_field / trace.sphere_trace) on distance_fn(pos float32 [M, 3]) -> D [M]: (state, evaluations)."""
    st = begin(origins, dirs, t_near)
    evaluations = 0
    for _ in range(max_steps):
        index, pos = compact(origins, dirs, st)
        if index.size == 0:
            break
        evaluations += index.size
        advance(st, index, distance_fn(pos), threshold, step_scale, min_step, t_far)
    finish(st)
    for _ in range(refine):
        index, pos = bisect_points(origins, dirs, st)
        if index.size == 0:
            break
        evaluations += index.size
        bisect_update(st, index, distance_fn(pos), threshold)
    return st, evaluations


def same_bits(a, b):
    """Equality of two arrays as stored (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def sphere_entry_depth(origins, dirs, radius):
    """float64 depth at which the ray o + t d enters the sphere |x| = radius (NaN for a ray that misses it) and the ray's impact
    parameter (distance of the line from the centre)."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    dd = (d * d).sum(1)
    tc = -(o * d).sum(1) / dd                                   # depth of the point nearest the centre
    b2 = ((o + tc[:, None] * d) ** 2).sum(1)                    # impact parameter squared
    with np.errstate(invalid="ignore"):
        half = np.sqrt((radius * radius - b2) / dd)
    return tc - half, np.sqrt(b2)


# ---- scenes and ray sets shared by the host and the GPU tests ----
SPHERE_R, TORUS_MAJOR, TORUS_MINOR = 0.5, 0.8, 0.12


def scene_distance(pos, xp=np):
    """Distance to a sphere of radius 0.5 at the origin plus a torus (major radius 0.8, minor 0.12) in the xz plane; xp = numpy or torch
    (the GPU test evaluates it with torch on the device: whatever it returns IS the distance array of the step)."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    sphere = xp.sqrt(x * x + y * y + z * z) - SPHERE_R
    ring = xp.sqrt(x * x + z * z) - TORUS_MAJOR
    torus = xp.sqrt(ring * ring + y * y) - TORUS_MINOR
    return xp.minimum(sphere, torus)


def scene_rays(n, t_near, threshold, seed=0):
    """n rays towards the scene from a shell of radius 3: aimed at random points of a ball of radius 1.3 (hits and misses), and by index
    modulo 16: rays that START inside the level set (o + t_near d at the centre of the sphere), rays grazing the sphere's level set just
    inside / just outside, and rows with a NaN or Inf origin or direction component."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = 3.0 * v
    target = rng.standard_normal((n, 3)); target *= (1.3 * rng.random(n) ** (1 / 3) / np.linalg.norm(target, axis=1))[:, None]
    side = np.cross(v, rng.standard_normal((n, 3))); side /= np.linalg.norm(side, axis=1, keepdims=True)
    k = np.arange(n) % 16
    graze = (SPHERE_R + threshold) * np.where(k == 3, 1.0 - 1e-4, 1.0 + 1e-4)
    target = np.where(((k == 3) | (k == 4))[:, None], side * graze[:, None], target)
    d = target - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.where((k == 5)[:, None], -t_near * d, o)              # starts inside: HIT with 0 steps
    o, d = o.astype(F), d.astype(F)
    if n >= 16:
        o[k == 6, 0] = np.nan; d[k == 7, 1] = np.nan; o[k == 8, 2] = np.inf; d[k == 9, 0] = -np.inf
    return o, d


def sphere_rays(n, seed=1):
    """n unit rays from a shell of radius 3 whose impact parameters cover [0, 1.6 SPHERE_R] evenly in area (hits and clear misses)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    side = np.cross(v, rng.standard_normal((n, 3))); side /= np.linalg.norm(side, axis=1, keepdims=True)
    b = 1.6 * SPHERE_R * np.sqrt(rng.random(n))
    d = side * b[:, None] - 3.0 * v; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (3.0 * v).astype(F), d.astype(F)


def check_sphere_closed_form(o, d, st, threshold, min_step, refine):
    """The closed-form gate of the sphere scene (step_scale 1): every ray with impact parameter <= 0.9 (R + tau) is HIT at
    t_tau <= t <= t_tau + min_step 2^-refine + 1e-5, t_tau the float64 entry depth of the sphere of radius R + tau; every ray with impact
    parameter >= R + tau + 1e-5 is MISS.  (1e-5: ten times the float32 rounding of the distance at t ~ 3, times 1 / cos of the incidence
    <= 2.3.)  Returns the figures it asserted on."""
    tau = float(F(threshold))
    t_tau, b = sphere_entry_depth(o, d, SPHERE_R + tau)
    inner, outer = b <= 0.9 * (SPHERE_R + tau), b >= SPHERE_R + tau + 1e-5
    assert inner.sum() > 0.2 * len(b) and outer.sum() > 0.2 * len(b)
    t = st["t"].astype(np.float64)
    over = t[inner] - t_tau[inner]
    figures = dict(n_inner=int(inner.sum()), n_outer=int(outer.sum()), min_over=float(over.min()), max_over=float(over.max()),
                   bound=float(min_step) * 2.0 ** -refine + 1e-5)
    print("closed form:", figures)
    assert (st["status"][inner] == HIT).all(), np.unique(st["status"][inner], return_counts=True)
    assert over.min() >= 0.0 and over.max() <= figures["bound"], figures
    assert (st["status"][outer] == MISS).all(), np.unique(st["status"][outer], return_counts=True)
    return figures
