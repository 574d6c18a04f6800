"""A seeded corpus of ray casts and sweeps with a stated purpose, the queries' counterpart of tests/contact_corpus.py: every branch of the
reference's ray tests (oracle/mgf_collision.hpp:51-149, restated for the device in mgf_amd/csrc/dev_geom.h) is the aim of a named family
here, tests/test_query_corpus.py measures with gcov that the corpus reaches them, and the families aimed at the acceleration structure in
front of those tests (the query grid's walk, mgf_amd/csrc/k_query.h; the batch's bounding-sphere reject, k_batch_query.h) are laid over
the scale ladder of the contact corpus.  Generators only: numpy, seeded, no GPU.

A ray case is a row of RAY_DTYPE - CASE_DTYPE and a `dt`: the target is `a`, the particle's origin the centre of `b` (a sphere of radius
0, so that contact_corpus.place moves and scales it as it does every point), its direction `vb`.  A sweep case is a row of CASE_DTYPE as the
contact corpus makes it: `a` the resting target, `b` the cast, `vb` its delta (`va` is not used: the target rests).

  ray_families()        per target kind, over the ladder;  direction_ladder()  max|d_k| from 1e-24 to 1e30 over hits and off-line targets
  sweep_base()          contact_corpus's moving-pair and moving-triangle families as casts, and the sweeps' own edge cases
  ray_world(name, rung) a world of the corpus planted on the lattice with its particles (the walk families included)
  sweep_world(rung)     the sweep cases planted on the lattice, and the casts aimed at the grid's block walk
  band_scan()           the scan that measured the direction band of include/mgf_hip.h (python -m tests.query_corpus)
"""
import numpy as np

from oracle.oracle import COMPONENT_DTYPE, SHAPE_DTYPE
from tests import contact_corpus as CC
from tests.contact_corpus import CAPSULE, LADDER, PITCH, SPHERE, TRIANGLE, WORLD_RUNGS, over_ladder, place, plant, roll_axes  # noqa: F401

INF = np.float32(np.inf)
RAY_DTYPE = np.dtype(CC.CASE_DTYPE.descr + [("dt", "<f4")])
FAMILIES = []          # names; RAY_DTYPE.family indexes this list (the sweep cases keep contact_corpus.FAMILIES)


def _fam(name):
    if name not in FAMILIES:
        FAMILIES.append(name)
    return FAMILIES.index(name)


def family_names(cases):
    return np.array(FAMILIES)[cases["family"]]


def rays(family, target, p, d, dt=INF):
    """(n,) RAY_DTYPE: particles (p, d, dt) against the shapes `target`"""
    n = len(target)
    out = np.zeros(n, RAY_DTYPE)
    out["family"] = _fam(family)
    out["a"] = target
    out["b"]["kind"] = SPHERE
    out["b"]["v"][:, :3] = np.asarray(p, np.float64).reshape(n, 3).astype(np.float32)
    out["vb"] = np.asarray(d, np.float64).reshape(n, 3).astype(np.float32)
    out["hv"] = 2
    out["dt"] = dt
    return out


def origin(cases):
    return np.ascontiguousarray(cases["b"]["v"][:, :3])


_unit, _perp, _shape = CC._unit, CC._perp, CC._shape


# ---- spheres (mgf_collision.hpp:51-62) ------------------------------------------------------------------------------------------------
def sphere_rays(S, rng):
    """for every sphere of S one particle of each family"""
    n = len(S)
    c, r = S["v"][:, :3].astype(np.float64), S["v"][:, 3].astype(np.float64)[:, None]
    out = []
    u, w = _unit(rng, n), _unit(rng, n)
    out.append(rays("sphere_origin_inside", S, c + u * r * rng.uniform(0.0, 0.95, (n, 1)), w * rng.uniform(0.2, 3.0, (n, 1))))       # c < 0: t clamped to 0
    out.append(rays("sphere_origin_at_centre", S, c, w))
    out.append(rays("sphere_origin_on_surface", S, c + u * r, w * rng.uniform(0.2, 3.0, (n, 1))))                                   # c = 0 up to rounding
    out.append(rays("sphere_pointing_away", S, c + u * r * rng.uniform(1.05, 4.0, (n, 1)), u + 0.4 * w))                             # c > 0 && b > 0
    side = _perp(rng, u)
    for k in (-3, -1, 0, 1, 3):      # discr within a few ulps of 0: the line passes at r (1 + k 2^-23) from the centre
        off = r * (1.0 + k * 2.0 ** -23)
        out.append(rays("sphere_tangent_ulps", S, c + side * off - u * r * rng.uniform(1.5, 4.0, (n, 1)), u * rng.uniform(0.5, 2.0, (n, 1))))
    aim = c + _unit(rng, n) * r * rng.uniform(0.0, 0.9, (n, 1))
    p = c + u * r * rng.uniform(1.2, 5.0, (n, 1))
    out.append(rays("sphere_hit", S, p, (aim - p) * rng.uniform(0.3, 3.0, (n, 1))))
    out.append(rays("sphere_segment_short", S, p, (aim - p) * rng.uniform(0.05, 0.5, (n, 1)), 1.0))
    aim = c + side * r * rng.uniform(1.1, 3.0, (n, 1))
    out.append(rays("sphere_miss", S, p, aim - p))
    out.append(rays("sphere_dt_zero", S, np.where(rng.random((n, 1)) < 0.5, p, c + u * r * 0.5), w, 0.0))
    return np.concatenate(out)


# ---- capsules (mgf_collision.hpp:65-112) ----------------------------------------------------------------------------------------------
def capsule_rays(K, rng, axis_aligned=False):
    n = len(K)
    a, d, r = K["v"][:, :3].astype(np.float64), K["v"][:, 3:6].astype(np.float64), K["v"][:, 6].astype(np.float64)[:, None]
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    ax = d / np.maximum(ln, 1e-30)
    side = _perp(rng, np.where(ln > 0, ax, (1.0, 0.0, 0.0)))
    out = []
    tag = "_exact" if axis_aligned else ""
    # |a| < epsilon by parallelism (exact when the axis is a coordinate axis: d is a multiple of it), :72-88
    for name, s0 in (("before", -rng.uniform(0.2, 2.0, (n, 1)) - r / np.maximum(ln, 1e-30)), ("beyond", 1.0 + rng.uniform(0.2, 2.0, (n, 1)) + r / np.maximum(ln, 1e-30)),
                     ("between", rng.uniform(0.05, 0.95, (n, 1)))):
        for h in (0.0, 0.5, 1.5):        # on the axis, inside the radius, outside it
            p = a + d * s0 + side * r * h
            for sgn in (1.0, -1.0):
                out.append(rays(f"capsule_parallel{tag}_{name}", K, p, d * sgn * np.round(rng.uniform(1.0, 3.0, (n, 1)))))
    # ... by near parallelism
    tilt = d + side * ln * 10.0 ** rng.uniform(-6.0, -3.5, (n, 1))
    out.append(rays("capsule_near_parallel", K, a - d * rng.uniform(0.5, 2.0, (n, 1)) + side * r * rng.uniform(0.0, 1.2, (n, 1)), tilt))
    out.append(rays("capsule_near_parallel", K, a + d * rng.uniform(1.5, 3.0, (n, 1)) + side * r * rng.uniform(0.0, 1.2, (n, 1)), -tilt))
    # the general branch (:89-111): the cylinder, t < 0, either end cap and their early returns
    mid = a + d * rng.uniform(0.1, 0.9, (n, 1))
    u = _unit(rng, n)
    p = mid + side * r * rng.uniform(1.5, 5.0, (n, 1)) + ax * ln * rng.uniform(-0.3, 0.3, (n, 1))
    out.append(rays("capsule_cylinder_hit", K, p, (mid + _unit(rng, n) * r * 0.5 - p) * rng.uniform(0.4, 2.0, (n, 1))))
    out.append(rays("capsule_cylinder_miss", K, p, np.cross(ax, side) + 0.2 * u))                               # discr < 0
    out.append(rays("capsule_origin_inside", K, mid + side * r * rng.uniform(0.0, 0.9, (n, 1)), u + 0.3 * side))      # t < 0
    out.append(rays("capsule_cylinder_behind", K, p, p - mid + 0.3 * np.cross(ax, side)))                       # t < 0, pointing away
    for name, end, away in (("a", a, -ax), ("b", a + d, ax)):
        tip = end + away * r * rng.uniform(1.3, 4.0, (n, 1)) + side * r * rng.uniform(0.0, 0.8, (n, 1))
        out.append(rays(f"capsule_end_{name}_hit", K, tip, (end - tip) + 0.1 * side * r))                        # falls through to the end sphere
        out.append(rays(f"capsule_end_{name}_inside", K, end + away * r * rng.uniform(0.1, 0.9, (n, 1)), u))         # inside the end sphere
        # crosses the infinite cylinder beyond the end, then passes the end sphere by (discr2 < 0) or points away from it (the early return)
        far = end + away * (r * rng.uniform(1.5, 3.0, (n, 1))) + side * r * rng.uniform(2.0, 4.0, (n, 1))
        out.append(rays(f"capsule_end_{name}_passes_by", K, far, -side + 0.05 * away))
        out.append(rays(f"capsule_end_{name}_pointing_away", K, far, -side * 0.2 + away))
        out.append(rays(f"capsule_end_{name}_slanted", K, far, -side - 0.6 * away + 0.1 * u))
    return np.concatenate(out)


def _capsules(rng, n, axis_aligned=False, length=(0.3, 1.5)):
    c = rng.uniform(-2, 2, (n, 3))
    if axis_aligned:
        d = np.eye(3)[rng.integers(0, 3, n)] * (rng.integers(2, 9, (n, 1)) / 4.0) * rng.choice([-1.0, 1.0], (n, 1))
        c = np.round(c * 4) / 4
    else:
        d = _unit(rng, n) * rng.uniform(length[0], length[1], (n, 1))
    return _shape(CAPSULE, c, d, rng.uniform(0.3, 0.9, n))


def small_capsule_rays(rng, n):
    """the |a| < epsilon branch reached by smallness alone: dd * nn < 1e-6 although the ray is nowhere near parallel - short capsules and
    short segments at unit scale (the x0.05 rungs of the ladder do the same to every capsule family)"""
    K = _shape(CAPSULE, rng.uniform(-2, 2, (n, 3)), _unit(rng, n) * rng.uniform(0.005, 0.03, (n, 1)), rng.uniform(0.01, 0.05, n))
    a, d, r = K["v"][:, :3].astype(np.float64), K["v"][:, 3:6].astype(np.float64), K["v"][:, 6].astype(np.float64)[:, None]
    out = []
    for s0, name in ((-3.0, "md_negative"), (4.0, "md_beyond"), (0.5, "md_between")):
        p = a + d * s0 + _unit(rng, n) * r * rng.uniform(0.0, 3.0, (n, 1))
        aim = a + d * rng.uniform(0, 1, (n, 1))
        dirn = np.cross(d, _unit(rng, n)) + (aim - p)
        dirn *= (rng.uniform(0.005, 0.03, (n, 1)) / np.linalg.norm(dirn, axis=1, keepdims=True))
        out.append(rays(f"capsule_small_{name}", K, p, dirn, np.where(rng.random(n) < 0.5, INF, np.float32(1.0))))
    return np.concatenate(out)


def zero_length_capsule_rays(rng, n):
    K = _shape(CAPSULE, rng.uniform(-2, 2, (n, 3)), np.zeros((n, 3)), rng.uniform(0.3, 0.9, n))
    a, r = K["v"][:, :3].astype(np.float64), K["v"][:, 6].astype(np.float64)[:, None]
    u = _unit(rng, n)
    p = a + u * r * rng.uniform(0.0, 3.0, (n, 1))
    return rays("capsule_zero_length", K, p, (a - p) + 0.2 * _unit(rng, n))


# ---- triangles (ray_plane :115-122, ray_polygon :125-129, contains :35-42) --------------------------------------------------------------
def triangle_rays(T, rng, floor=False):
    n = len(T)
    a, b, c = (T["v"][:, k:k + 3].astype(np.float64) for k in (0, 3, 6))
    nrm = np.cross(b - a, c - a)
    nl = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm / np.maximum(nl, 1e-30)
    e = b - a
    out = []
    tag = "_floor" if floor else ""
    w = rng.dirichlet((2.0, 2.0, 2.0), n)
    inside = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    h = rng.uniform(0.3, 3.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    p = inside + nrm * h + (c - a) * rng.uniform(-0.3, 0.3, (n, 1))
    out.append(rays(f"triangle_face_hit{tag}", T, p, (inside - p) * rng.uniform(0.5, 2.0, (n, 1))))
    out.append(rays(f"triangle_segment_short{tag}", T, p, (inside - p) * rng.uniform(0.1, 0.9, (n, 1)), 1.0))
    out.append(rays(f"triangle_behind{tag}", T, p, p - inside))                                                    # t <= 0
    out.append(rays(f"triangle_origin_in_plane{tag}", T, inside, nrm + 0.3 * e))                                    # t = 0: "<= 0"
    out.append(rays(f"triangle_in_plane{tag}", T, inside - e * 2.0, e))                                             # denom == 0 when exact
    out.append(rays(f"triangle_parallel{tag}", T, inside + nrm * h - e * 2.0, e))
    outside = a + (a - 0.5 * (b + c)) * rng.uniform(0.2, 1.5, (n, 1))
    out.append(rays(f"triangle_plane_hit_outside{tag}", T, outside + nrm * h, -nrm * h * 2.0))
    # on an edge, on a vertex and a few ulps to either side of each (ulps of the coordinates' magnitude, along the in-plane outward direction)
    ctr = (a + b + c) / 3.0
    V = [a, b, c]
    for i in range(3):
        on_edge = V[i] + (V[(i + 1) % 3] - V[i]) * rng.uniform(0.1, 0.9, (n, 1))
        for name, on in ((f"edge{i}", on_edge), (f"vertex{i}", V[i])):
            outward = on - ctr
            outward /= np.maximum(np.linalg.norm(outward, axis=1, keepdims=True), 1e-30)
            scale = np.maximum(np.abs(on).max(axis=1, keepdims=True), 1.0) * 2.0 ** -23
            for k in (-4, -1, 0, 1, 4):
                tgt = on + outward * scale * k
                pp = tgt + nrm * h
                out.append(rays(f"triangle_{name}_ulps{tag}", T, pp, (tgt - pp) * 2.0))
    return np.concatenate(out)


def _floor_triangles(rng, n):
    ta, tb, tc, *_ = CC._floor_tris(rng, n, int(rng.integers(0, 3)))
    return _shape(TRIANGLE, ta, tb, tc)


def _random_triangles(rng, n):
    return _shape(TRIANGLE, *CC._rand_tris(rng, n))


def degenerate_triangle_rays(rng):
    """the degenerate triangles of contact_corpus.degenerate_triangles: whatever the oracle answers (NaN included) is the expectation"""
    T = CC.degenerate_triangles()["a"]
    n = len(T)
    a = T["v"][:, :3].astype(np.float64)
    p = a + _unit(rng, n) * rng.uniform(0.5, 3.0, (n, 1))
    return rays("triangle_degenerate", T, p, (a - p) + rng.normal(0, 0.2, (n, 3)))


# ---- the hit's own t as dt ----------------------------------------------------------------------------------------------------------
def oracle_answers(cases, dt=None):
    """(hit, point, t) of the oracle's single test for every case"""
    from oracle import oracle as O
    return O.intersection_batch(origin(cases), cases["vb"], cases["dt"] if dt is None else dt, cases["a"])


def dt_edges(cases):
    """for every case that hits at a finite t > 0: the same particle with dt just below, at and just above the hit's own t"""
    hit, _, t = oracle_answers(cases, INF)
    m = (hit == 1) & np.isfinite(t) & (t > 0)
    src, t = cases[m], t[m]
    names = family_names(src)
    out = []
    for how, dt in (("below", np.nextafter(t, np.float32(0))), ("at", t), ("above", np.nextafter(t, INF))):
        c = src.copy()
        c["dt"] = dt
        for f in set(names.tolist()):
            c["family"][names == f] = _fam(f"dt_{how}_hit:" + f.split("_")[0])
        out.append(c)
    return np.concatenate(out)


# ---- the direction ladder ------------------------------------------------------------------------------------------------------------
DIRECTIONS = np.array([(1.0, 0.0, 0.0), (0.7, 0.5, -0.3), (-0.6, 1.0, 0.8)])      # max |component|: 1, 0.7, 1
DECADES = list(range(-24, 31, 2))


def direction_ladder(seed=31, n=6):
    """max|d_k| from 1e-24 to 1e30, every other decade, in three directions: targets on the line (a hit at unit scale) and targets well
    off it (the evidence of the issue: origin 0, a sphere and a capsule at (50, 30, -20)); dt = inf"""
    rng = np.random.default_rng(seed)
    out = []
    for k, u in enumerate(DIRECTIONS):
        un = u / np.linalg.norm(u)
        for on_line in (True, False):
            p = rng.uniform(-1, 1, (n, 3))
            dist = rng.uniform(3.0, 60.0, (n, 1))
            side = _perp(rng, np.tile(un, (n, 1)))
            c = p + un * dist + side * (0.2 if on_line else 1.0) * np.where(on_line, rng.uniform(0, 1, (n, 1)), rng.uniform(4.0, 40.0, (n, 1)))
            c[0] = (50.0, 30.0, -20.0) if not on_line else c[0]
            p[0] = 0.0 if not on_line else p[0]
            S = _shape(SPHERE, c, np.full(n, 0.5))
            K = _shape(CAPSULE, c - np.array([0, 0.5, 0]), np.tile([0.0, 1.0, 0.0], (n, 1)), np.full(n, 0.5))
            tri_c = c if on_line else c + side * 3.0
            T = _shape(TRIANGLE, tri_c + np.cross(un, side) * 1.5, tri_c - np.cross(un, side) * 1.5 + side * 1.5, tri_c - np.cross(un, side) * 1.5 - side * 1.5)
            for e in DECADES:
                d = np.tile(u * 10.0 ** e, (n, 1))
                for tgt, kind in ((S, "sphere"), (K, "capsule"), (T, "triangle")):
                    r = rays(f"direction_ladder_{'on' if on_line else 'off'}_line:{kind}", tgt, p, d)
                    r["hv"] = 2 + 4 * (e - DECADES[0]) // 2      # (the decade, for the band scan: bits 2.. of hv)
                    out.append(r)
    return np.concatenate(out)


def decade_of(cases):
    return DECADES[0] + 2 * (cases["hv"].astype(np.int64) >> 2)


# ---- the pair-level ray corpus -----------------------------------------------------------------------------------------------------------
def ray_base(seed=21, n=24):
    """every ray family at unit scale around the origin"""
    rng = np.random.default_rng(seed)
    S = _shape(SPHERE, rng.uniform(-2, 2, (n, 3)), rng.uniform(0.3, 1.2, n))
    parts = [sphere_rays(S, rng), capsule_rays(_capsules(rng, n), rng), capsule_rays(_capsules(rng, n, axis_aligned=True), rng, axis_aligned=True),
             small_capsule_rays(rng, n), zero_length_capsule_rays(rng, n), triangle_rays(_random_triangles(rng, n), rng),
             triangle_rays(_floor_triangles(rng, n), rng, floor=True), degenerate_triangle_rays(rng)]
    base = np.concatenate(parts)
    floor = np.array([f.endswith("_floor") for f in family_names(base)])
    return roll_axes(base, np.where(floor, np.arange(len(base)) % 3, 0))


def ray_families(seed=22):
    """the families over the ladder, with the hit's own t as dt, and the direction ladder (rung 0 only: it is its own ladder)"""
    FAMILIES.clear()
    base = ray_base()
    lad = over_ladder(base, np.random.default_rng(seed))
    return np.concatenate([lad, dt_edges(lad), direction_ladder()])


# ---- sweeps ------------------------------------------------------------------------------------------------------------------------------
def sweep_base(per_family=3, seed=23):
    """contact_corpus's moving-pair and moving-triangle families at rung 0 (a the resting target, b the cast, vb its delta), thinned to
    `per_family` cases of each family and type, and the sweeps' own edge cases"""
    c = CC.base_cases(CC.TYPES, per_family=per_family, seed=seed)
    rng = np.random.default_rng(seed)
    n = 6
    extra = []
    ctr = rng.uniform(-2, 2, (n, 3))
    S = _shape(SPHERE, ctr, rng.uniform(0.3, 0.9, n))
    z = np.zeros((n, 3))
    extra.append(CC._cases("sweep_sphere_equal_centres", S, _shape(SPHERE, ctr, rng.uniform(0.2, 0.6, n)), z, z))
    extra.append(CC._cases("sweep_sphere_equal_centres_moving", S, _shape(SPHERE, ctr, rng.uniform(0.2, 0.6, n)), z, _unit(rng, n)))
    u = _unit(rng, n)
    for name, delta in (("sweep_delta_zero_overlapping", z), ("sweep_delta_tiny", u * 1e-23), ("sweep_starts_overlapping", u * rng.uniform(0.2, 2.0, (n, 1)))):
        for kb in (SPHERE, CAPSULE):
            at = ctr + u * S["v"][:, 3:4] * rng.uniform(0.2, 1.2, (n, 1))
            B = _shape(SPHERE, at, np.full(n, 0.4)) if kb == SPHERE else _shape(CAPSULE, at, _unit(rng, n) * 0.8, np.full(n, 0.3))
            extra.append(CC._cases(name, S, B, z, delta))
    # a capsule at rest beside a capsule with parallel axes (the 0 / 0 quirk DESIGN section 3 records for faces)
    ax = np.eye(3)[rng.integers(0, 3, n)]
    la = rng.integers(2, 9, (n, 1)) / 4.0
    a0 = np.round(ctr * 4) / 4
    K = _shape(CAPSULE, a0, ax * la, np.full(n, 0.5))
    for h in (0.75, 1.5, 6.0):
        extra.append(CC._cases("sweep_capsule_at_rest_parallel", K, _shape(CAPSULE, a0 + np.roll(ax, 1, axis=1) * h, ax * la, np.full(n, 0.5)), z, z))
    extra = np.concatenate(extra)
    extra["hv"] = 2
    c = c.copy()
    c["va"] = 0
    c["hv"] = 2
    return np.concatenate([c, extra])


def sweep_oracle(cases):
    """(contacts (n, 2), counts) of the oracle's single test: the target at rest, the cast moving"""
    from oracle import oracle as O
    return O.contacts_batch(cases["a"], np.zeros((len(cases), 3), np.float32), cases["b"], cases["vb"], np.full(len(cases), 2, np.uint8), slots=2)


# ---- the world form ------------------------------------------------------------------------------------------------------------------------
MAX_BODIES, MAX_QUERIES = 96, 4096
TIES = 8             # pairs of bodies with equal t (ray_world: spheres, mixed)
WORLDS = ["spheres", "mixed", "mixed_face_grid", "obstacle", "parts", "wide"]


def _grid_of(boxes_c, boxes_r, rmax):
    """The query grid as mgf_amd/csrc/host_query.inc lays it over the bodies' tight boxes (centre, half extent, f32): dict(lo, h, dims,
    margin, n_large).  rmax: the largest half extent a body's fat box had when it was added (tight + 0.25: bounds.rs, world.rs:233)."""
    f = np.float32
    h = f(2.0) * f(rmax)
    margin = f(1e-3) * h
    c, r = np.asarray(boxes_c, f), np.asarray(boxes_r, f)
    wide = ~np.all(f(2.0) * (r + margin) <= h, axis=1)
    if wide.all():
        return dict(lo=np.zeros(3, f), h=h, dims=np.zeros(3, np.int64), margin=margin, n_large=int(wide.sum()))
    lo = ((c - r) - margin)[~wide].min(axis=0)
    hi = ((c + r) + margin)[~wide].max(axis=0)
    margin = max(margin, f(4e-6) * f(max(np.abs(lo).max(), np.abs(hi).max())))
    cap = max(4096.0, 2.0 * int((~wide).sum()))
    while True:
        dims = np.minimum(np.floor((hi.astype(np.float64) - lo.astype(np.float64)) / float(h)) + 1.0, 1e9)
        if dims.prod() <= cap:
            break
        h = f(h * f(1.25))
    return dict(lo=(lo - f(margin)).astype(f), h=f(h), dims=dims.astype(np.int64) + 1, margin=f(margin), n_large=int(wide.sum()))


def comp_boxes(comps):
    """BoundedBy<AABB> of single components (bounds.rs:170-190) in f32"""
    f = np.float32
    cap = comps["tag"] == 1
    d = np.where(cap[:, None], comps["d"], f(0)).astype(f)
    m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=f)
    r = np.where(cap, comps["r"] + m * f(0.5), comps["r"]).astype(f)
    c = np.where(cap[:, None], comps["p"] + d * f(0.5), comps["p"]).astype(f)
    return c, np.repeat(r[:, None], 3, axis=1)


def world_grid(world):
    """the restated query grid of a world of single-component bodies"""
    c, r = comp_boxes(world["comps"])
    # the fat box a body is added with: its box combined with itself (the swept bound of a body at rest, bounds.rs:60-68 and :113-130),
    # whose half extent (upper - lower) / 2 carries the rounding of the coordinates, and the fat pad 0.25
    swept = ((c + r) - (c - r)) / np.float32(2.0)
    return _grid_of(c, r, float((swept + np.float32(0.25)).max()))


def _particles(family, p, d, dt=INF):
    n = len(p)
    return rays(family, np.zeros(n, SHAPE_DTYPE), p, d, dt)


def walk_rays(world, rng, size):
    """particles aimed at the grid, not at a shape: see the family names.  `size`: the rung's scale"""
    G = world_grid(world)
    lo, h, dims = G["lo"].astype(np.float64), float(G["h"]), G["dims"]
    hi = lo + dims * h
    out = []
    n = 12

    def face(k, i):
        return lo[k] + h * i
    for k in range(3):       # running exactly in a cell-face plane: d_k = 0, p_k on a face (f32 of it), across the grid along another axis
        j = (k + 1) % 3
        p = np.stack([rng.uniform(lo, hi) for _ in range(n)])
        p[:, k] = np.float32(face(k, rng.integers(0, dims[k] + 1, n)))
        p[:, j] = lo[j] - 2.0 * h
        d = np.zeros((n, 3)); d[:, j] = 1.0
        out.append(_particles("walk_in_face_plane", p, d * size))
        # along a cell edge: two coordinates on faces
        m = (k + 2) % 3
        p2 = p.copy(); p2[:, m] = np.float32(face(m, rng.integers(0, dims[m] + 1, n)))
        out.append(_particles("walk_along_cell_edge", p2, d * size))
    # through cell corners on the diagonal, entering at the grid's corner
    for sgn in ((1, 1, 1), (1, -1, 1), (-1, 1, -1)):
        s = np.array(sgn, np.float64)
        corner = np.where(s > 0, lo, hi)
        out.append(_particles("walk_corner_diagonal", np.tile(corner - s * h * 2.0, (2, 1)), np.tile(s * size, (2, 1))))
    # from outside through a face, an edge and a corner; from 1e5 (times the rung's scale of things) outside, pointing in
    tgt = world["aim"][rng.integers(0, len(world["aim"]), 4 * n)]
    for name, mask in (("face", (1, 0, 0)), ("edge", (1, 1, 0)), ("corner", (1, 1, 1))):
        mk = np.roll(np.array(mask, np.float64), int(rng.integers(0, 3)))
        p = tgt[:n] + mk * (hi - lo + 3.0 * h) * rng.choice([-1.0, 1.0], (n, 3))
        out.append(_particles(f"walk_enters_through_{name}", p, tgt[:n] - p))
    for dist in (3e3, 2e4, 1e5):      # the `fat` rule (4e-7 (|p| + dmax t1) > 0.25 margin) below and above its threshold
        u = _unit(rng, n)
        p = tgt[n:2 * n] + u * dist * max(size, 0.05)
        out.append(_particles("walk_far_origin", p, tgt[n:2 * n] - p))
        out.append(_particles("walk_far_origin_unit_d", p, -u))
    # far origins whose line passes BESIDE the grid's box, parallel to a face and 1 .. 30 sizes outside it, and segments from far away
    # aimed at a body that end short of the box: no cell is theirs, yet a body within the tube of the line answers
    m = 3 * n
    k = rng.integers(0, 3, m)
    j = (k + 1) % 3
    p = np.stack([rng.uniform(lo, hi) for _ in range(m)])
    p[np.arange(m), k] = hi[k] + rng.uniform(1.0, 30.0, m) * size
    dist = np.where(np.arange(m) % 2 == 0, 1e5, 2e4) * max(size, 0.05)
    p[np.arange(m), j] = lo[j] - dist
    d = np.zeros((m, 3)); d[np.arange(m), j] = dist + (hi - lo)[j] * rng.uniform(0.0, 1.0, m)
    out.append(_particles("walk_far_origin_beside_the_grid", p, d * np.where(np.arange(m) % 3 == 0, 1.0, 2.0)[:, None], np.where(np.arange(m) % 3 == 0, 1.0, INF)))
    u = _unit(rng, n)
    p = tgt[3 * n:4 * n] + u * 1e5 * max(size, 0.05)
    short = (np.linalg.norm(hi - lo) + rng.uniform(1.0, 30.0, n) * size) / (1e5 * max(size, 0.05))
    out.append(_particles("walk_far_segment_ends_short_of_the_grid", p, (tgt[3 * n:4 * n] - p) * (1.0 - short)[:, None], 1.0))
    # from a few thousand sizes away, almost along a face of the box: the line runs beside the box for many cells before it enters or after
    # it leaves, and there passes just outside a body that lies at that face - the hit is at a point of the line outside the box
    m = 4 * n
    k = rng.integers(0, 3, m)
    j = (k + 1 + rng.integers(0, 2, m)) % 3
    side = rng.choice([-1.0, 1.0], m)
    sph = np.nonzero(world["comps"]["tag"] == 0)[0]
    sc_, sr_ = world["comps"]["p"][sph].astype(np.float64), world["comps"]["r"][sph].astype(np.float64)
    # a sphere whose surface is the outermost, or nearly, on that side: the line's point abreast of it lies just off its surface
    pick = np.array([np.argsort(side[i] * sc_[:, k[i]] + sr_)[-1 - rng.integers(0, min(3, len(sph)))] for i in range(m)])
    at = sc_[pick].copy()
    off_box = 2.0 * float(G["margin"]) if 2.0 * float(G["margin"]) < 0.5 * size else 0.0      # (beyond the box's own pad, where a hit can be)
    at[np.arange(m), k] += side * (sr_[pick] + off_box + rng.uniform(0.01, 0.3, m) * size)
    dist = rng.uniform(1.5e3, 8e3, m) * size
    slope = rng.uniform(0.007, 0.03, m) * rng.choice([-1.0, 1.0], m)
    d = np.zeros((m, 3)); d[np.arange(m), j] = -1.0; d[np.arange(m), k] = slope
    d *= rng.choice([-1.0, 1.0], (m, 1))
    out.append(_particles("walk_grazes_a_face_from_afar", at - d * dist[:, None], d * size))
    # missing the grid by an ulp: along a face of its box, just outside and just inside
    for k in range(3):
        j = (k + 1) % 3
        p = np.stack([rng.uniform(lo, hi) for _ in range(n)])
        edge = np.float32(np.where(rng.random(n) < 0.5, lo[k], hi[k]))
        p[:, k] = np.where(np.arange(n) % 2 == 0, np.nextafter(edge, -INF), np.nextafter(edge, INF))
        p[:, j] = lo[j] - h
        d = np.zeros((n, 3)); d[:, j] = 1.0
        out.append(_particles("walk_grazes_grid_box", p, d * size))
    # segments that end inside the first cell; a hit in the last cell of the walk (aimed at the bodies of the far side from far away)
    p = tgt[2 * n:3 * n] + _unit(rng, n) * h * 3.0
    out.append(_particles("walk_segment_ends_in_first_cell", p, (tgt[2 * n:3 * n] - p) * rng.uniform(0.01, 0.2, (n, 1)), 1.0))
    far_side = world["aim"][np.argsort(world["aim"][:, 0])[-n:]]
    p = far_side.copy(); p[:, 0] = lo[0] - 2.0 * h
    p[:, 1:] += rng.normal(0, 0.05 * size, (len(p), 2))
    out.append(_particles("walk_hit_in_last_cell", p, far_side - p))
    return np.concatenate(out)


def _targets_of(cases):
    """one body (or face) per case: its target"""
    return CC._comp(cases["a"])


def ray_world(name, rung, seed=41):
    """A world of the corpus at one rung: dict(comps, mesh, obstacle (a list of component arrays), compound, rays (RAY_DTYPE: the particle
    fields), families (a name per particle), aim, offset, size).  Site k of the lattice holds target k - a sphere or a capsule as a body,
    a triangle as a face - and the particles of its families; besides them the walk families, rows of equal t, particles aimed from
    above as the older tests aim them, and the direction ladder.  Bodies rest."""
    FAMILIES.clear()
    o, s = LADDER[rung]
    rng = np.random.default_rng(seed + 7 * rung + WORLDS.index(name))
    which = WORLD_RUNGS.index(rung) if rung in WORLD_RUNGS else 0
    base = ray_base(n=32)
    kind = base["a"]["kind"]
    names = family_names(base)
    degenerate = names == "triangle_degenerate"
    # the targets: the distinct shapes of the base families, spheres and capsules as bodies, triangles as faces
    def distinct(m):
        seen, keep = set(), []
        for i in np.nonzero(m)[0]:
            key = base["a"][i].tobytes()
            if key not in seen:
                seen.add(key)
                keep.append(i)
        return np.array(keep, np.int64)
    sph, cap, tri = distinct(kind == SPHERE), distinct((kind == CAPSULE) & (names != "capsule_zero_length")), distinct((kind == TRIANGLE) & ~degenerate)
    if name == "spheres":
        bodies, faces = sph, tri[:0]
    elif name == "mixed_face_grid":
        bodies, faces = np.concatenate([sph[::4], cap[which % 8::8]]), tri
    else:
        bodies, faces = np.concatenate([sph[which % 2::2], cap[which % 2::2]]), tri[which % 4::4][:12]
    if name in ("obstacle", "parts"):
        bodies = bodies[:24]
    sel = np.concatenate([bodies, faces]).astype(np.int64)
    assert len(bodies) + 2 * TIES <= MAX_BODIES
    sites = CC._sites(len(sel), rung)
    site_of = {base["a"][i].tobytes(): k for k, i in enumerate(sel)}
    member = np.array([site_of.get(base["a"][i].tobytes(), -1) for i in range(len(base))])
    mine = base[member >= 0]
    placed = place(mine, sites[member[member >= 0]], s)
    tgt = place(base[sel], sites, s)
    comps = CC._comp(tgt["a"][:len(bodies)])
    w = dict(comps=comps, mesh=None, obstacle=None, compound=None, offset=o, size=s, rung=rung, name=name)
    nf = len(faces)
    if nf:
        w["mesh"] = dict(verts=tgt["a"]["v"][len(bodies):, :9].reshape(3 * nf, 3).astype(np.float32), faces=np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3),
                         pos=np.zeros(3, np.float32))
    c, r = comp_boxes(comps)
    w["aim"] = c.astype(np.float64)
    lo, hi = (c - r).min(axis=0).astype(np.float64), (c + r).max(axis=0).astype(np.float64)
    extra = []
    if name == "obstacle":
        # two obstacles beside the lattice: a row of spheres with two at the same place (equal t at two components), and a lone capsule
        ob = np.zeros(5, COMPONENT_DTYPE)
        at = np.array([lo[0] - 2.0 * PITCH * s, lo[1], lo[2]])
        ob["p"] = (at + np.array([(0, 0, 0), (0, 0, 0), (3, 0, 0), (0, 3, 0), (6, 1, 2)]) * s).astype(np.float32)
        ob["tag"] = [0, 0, 0, 0, 1]
        ob["d"][4] = np.float32((0, 2 * s, 0))
        ob["r"] = np.float32([0.5, 0.5, 0.7, 0.4, 0.5]) * np.float32(s)
        ob2 = np.zeros(1, COMPONENT_DTYPE)
        ob2["tag"], ob2["p"], ob2["d"], ob2["r"] = 1, np.float32(at + np.array([0, 12, 0]) * s), np.float32((2 * s, 0, 0)), np.float32(0.6 * s)
        w["obstacle"] = [ob, ob2]
        oc = np.concatenate([ob["p"], ob2["p"]]).astype(np.float64)
        m = 16
        t = oc[rng.integers(0, len(oc), m)]
        p = t + _unit(rng, m) * s * rng.uniform(2.0, 8.0, (m, 1))
        extra.append(_particles("obstacle_aimed", p, (t - p) + rng.normal(0, 0.2 * s, (m, 3))))
        extra.append(_particles("obstacle_segment_short", p, ((t - p) + rng.normal(0, 0.2 * s, (m, 3))) * rng.uniform(0.1, 1.2, (m, 1)), 1.0))    # the first node box beyond dt
        extra.append(_particles("obstacle_origin_in_node_box", t + rng.uniform(-0.4, 0.4, (m, 3)) * s, _unit(rng, m) * s))
        extra.append(_particles("obstacle_equal_t_two_components", np.tile(oc[0] + np.array([0, 5.0, 0]) * s, (4, 1)) + rng.uniform(-0.3, 0.3, (4, 3)) * s * [1, 0, 1],
                                np.tile([0, -s, 0], (4, 1))))
    if name == "parts":
        # bodies of 2 and of 4 parts beside the lattice: rows of spheres and capsules along z
        m2, m4 = 6, 4
        pc = np.zeros(2 * m2 + 4 * m4, COMPONENT_DTYPE)
        at = np.array([lo[0], hi[1] + 2.0 * PITCH * s, lo[2]])
        k = 0
        offs = [0]
        for b in range(m2 + m4):
            for j in range(2 if b < m2 else 4):
                pc["tag"][k] = (b + j) % 2
                pc["p"][k] = np.float32(at + np.array([b * 6.0, 0.0, j * 1.5]) * s)
                pc["d"][k] = np.float32((0, s, 0)) if pc["tag"][k] else 0
                pc["r"][k] = np.float32(0.5 * s)
                k += 1
            offs.append(k)
        w["compound"] = dict(comps=pc, offsets=np.array(offs, np.int64))
        t = pc["p"].astype(np.float64)
        m = len(t)
        p = t + (_unit(rng, m) + [0, 0.5, 0]) * s * rng.uniform(2.0, 8.0, (m, 1))
        extra.append(_particles("parts_aimed", p, (t - p) + rng.normal(0, 0.2 * s, (m, 3))))
        p = t + np.array([0, 0, -9.0]) * s       # along a body's row of parts: the first part answers, equal or not
        extra.append(_particles("parts_along_the_row", p, np.tile([0, 0, s], (m, 1))))
        w["aim"] = np.concatenate([w["aim"], t])
    if name == "wide":
        # Bodies wider than a cell (the grid's large list).  The cell is twice the largest fat half extent a body had when added, so the
        # widest body of a world is on the list only where the margin (1e-3 h) exceeds the fat pad 0.25: capsules 400 long, whatever the rung.
        # One lies across the top of the lattice and is the right answer for particles from above; one far below never is.
        mid = 0.5 * (lo + hi)
        big = np.zeros(2, COMPONENT_DTYPE)
        big["tag"] = 1
        big["p"] = np.float32([(mid[0] - 200.0, hi[1] + 6.0 * s, mid[2]), (mid[0], lo[1] - 40.0 * PITCH * s - 1000.0, mid[2] - 200.0)])
        big["d"] = np.float32([(400.0, 0, 0), (0, 0, 400.0)])
        big["r"] = np.float32(0.5 * s)
        w["comps"] = np.concatenate([comps, big])
        m = 16
        x = rng.uniform(mid[0] - 190.0, mid[0] + 190.0, m)
        p = np.stack([x, np.full(m, hi[1] + 20.0 * s), mid[2] + rng.uniform(-0.7, 0.7, m) * s], 1)
        extra.append(_particles("wide_body_answers", p, np.tile([0, -s, 0], (m, 1))))
        extra.append(_particles("wide_body_is_not_the_answer", w["aim"][:m] + np.array([3.0, -8.0, 0.3]) * s, np.tile([-3.0 * s, 8.0 * s, -0.3 * s], (m, 1))))
    # Equal t at two bodies: pairs of equal spheres mirrored about a particle's line, exact in f32 (every coordinate a multiple of a power
    # of two the rung's ulp divides), so both tests run the same arithmetic and report the same t and point, bit for bit; the answer is
    # the lower index.  The first of each pair stands in FRONT of the lattice's bodies and the second BEHIND them, len(bodies) + TIES
    # indices apart: other lanes of a batch's query and, from 64 apart, another wave.  In half the pairs the lower index is the upper sphere.
    # Two bodies that share a point of their surfaces as the entry of one line overlap, so the two of a pair share the cells of that
    # point ("equal t at bodies in different cells" cannot be built: the hit's cell files both); what differs is their place in a cell's
    # list, their lane and their wave.  And the ticks push overlapping bodies apart: the tie is held before the ticks only, after them the
    # pairs are ordinary bodies.
    if name in ("spheres", "mixed"):
        q = 2.0 ** np.floor(np.log2(s)) / 4.0
        base = np.round(np.array([lo[0], lo[1], lo[2] - 3.0 * PITCH * s]) / q) * q
        first, second = np.zeros(TIES, COMPONENT_DTYPE), np.zeros(TIES, COMPONENT_DTYPE)
        tp = np.zeros((TIES, 3))
        for k in range(TIES):
            at = base + np.array([0.0, 0.0, -16.0 * q * k])
            up = 1.0 if k % 2 else -1.0
            first["p"][k], second["p"][k] = np.float32(at + [16.0 * q, up * q, 0.0]), np.float32(at + [16.0 * q, -up * q, 0.0])
            tp[k] = at
        first["r"] = second["r"] = np.float32(3.0 * q)
        w["comps"] = np.concatenate([first, w["comps"], second])
        w["ties"] = (np.arange(TIES), np.arange(TIES) + TIES + len(comps))
        extra.append(_particles("equal_t_at_two_bodies", tp, np.tile([4.0 * q, 0.0, 0.0], (TIES, 1))))
        extra.append(_particles("equal_t_at_two_bodies", tp, np.tile([32.0 * q, 0.0, 0.0], (TIES, 1)), 1.0))
    extra.append(walk_rays(w, rng, s))
    # aimed from above at (near) the bodies, as the older tests do, and segments of them
    m = 64
    t = w["aim"][rng.integers(0, len(w["aim"]), m)] + rng.normal(0, 0.4 * s, (m, 3))
    p = t + (rng.normal(0, 1.0, (m, 3)) + [0, 8.0, 0]) * s
    extra.append(_particles("aimed_from_above", p, t - p))
    extra.append(_particles("aimed_from_above_segment", p, (t - p) * rng.uniform(0.3, 1.3, (m, 1)), 1.0))
    # the direction ladder at this world's scale: a few origins, every decade, three directions
    lad = []
    for u in DIRECTIONS:
        for e in DECADES:
            q = w["aim"][rng.integers(0, len(w["aim"]), 2)] - (u / np.linalg.norm(u)) * 4.0 * s + rng.normal(0, 0.2 * s, (2, 3))
            r_ = _particles("direction_ladder", q, np.tile(u * 10.0 ** e, (2, 1)))
            r_["hv"] = 2 + 4 * (e - DECADES[0]) // 2
            lad.append(r_)
    extra.append(np.concatenate(lad))
    allr = np.concatenate([placed] + extra)
    allr["rung"] = rung
    assert len(allr) <= MAX_QUERIES, len(allr)
    w["rays"] = allr
    w["casts"], w["cast_families"] = _world_casts(w, rng)
    w["families"] = np.array(FAMILIES)[allr["family"]]      # (FAMILIES is rebuilt by every generator: a world keeps its own names)
    return w


def _world_casts(w, rng, n=48):
    """casts for a world of particles: spheres and capsules from around the bodies (and the obstacles' and parts' components) aimed at
    others, short, long and at rest; for the world with wide bodies, casts onto the long capsule and casts wider than a cell.  Returns
    (CASE_DTYPE rows - b the cast, vb its delta - and a family name per cast)"""
    s = w["size"]
    aim = w["aim"]
    if w["obstacle"]:
        aim = np.concatenate([aim] + [ob["p"].astype(np.float64) for ob in w["obstacle"]])
    out, fam = [], []

    def add(name, tag, p, d, rad, delta):
        m = len(p)
        none = np.zeros(m, SHAPE_DTYPE)
        none["kind"] = TRIANGLE
        B = _shape(SPHERE, p, rad) if tag == 0 else _shape(CAPSULE, p, d, rad)
        c = np.zeros(m, CC.CASE_DTYPE)
        c["a"], c["b"], c["hv"] = none, B, 2
        c["vb"] = np.asarray(delta, np.float64).astype(np.float32)
        out.append(c)
        fam.extend([name] * m)
    for name, length in (("cast_short", (0.05, 0.9)), ("cast_long", (4.0, 20.0)), ("cast_at_rest", (0.0, 0.0))):
        for tag in (0, 1):
            src = aim[rng.integers(0, len(aim), n)] + (rng.normal(0, 0.4, (n, 3)) + [0.0, 1.5, 0.0]) * s
            tgt = aim[rng.integers(0, len(aim), n)] + rng.normal(0, 0.4, (n, 3)) * s
            if name == "cast_short":
                tgt = src - [0.0, 1.5 * s, 0.0] + rng.normal(0, 0.3, (n, 3)) * s
            u = tgt - src
            u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-30)
            ax = _unit(rng, n) * rng.uniform(0.3, 1.5, (n, 1)) * s
            add(name, tag, src - 0.5 * ax * tag, ax, rng.uniform(0.2, 0.6, n) * s, u * rng.uniform(length[0], length[1], (n, 1)) * s)
    if w["name"] == "wide":
        big = w["comps"][-2]
        m = 12
        on = big["p"].astype(np.float64) + big["d"].astype(np.float64) * rng.uniform(0.05, 0.95, (m, 1))
        add("cast_onto_the_wide_body", 0, on + [0.0, 3.0 * s, 0.0], None, np.full(m, 0.5 * s), np.tile([0.0, -4.0 * s, 0.0], (m, 1)))
        add("cast_onto_the_wide_body", 1, on + [0.0, 3.0 * s, -0.5 * s], np.tile([0.0, 0.0, s], (m, 1)), np.full(m, 0.3 * s), np.tile([0.0, -4.0 * s, 0.0], (m, 1)))
        t = aim[rng.integers(0, len(aim) - 2, m)]
        add("cast_wider_than_the_rest", 0, t + [0.0, 30.0 * s, 0.0], None, np.full(m, 8.0 * s), np.tile([0.0, -40.0 * s, 0.0], (m, 1)))
    return np.concatenate(out), np.array(fam)


def world_particles(w):
    """(p, d, dt) of a world's particles"""
    r = w["rays"]
    return origin(r), np.ascontiguousarray(r["vb"]), np.ascontiguousarray(r["dt"])


# ---- a world of casts --------------------------------------------------------------------------------------------------------------------------
def sweep_world(rung, seed=43):
    """The sweep cases planted on the lattice: the target of case k a body (a sphere or a capsule) or a face (a triangle) at site k, the
    cast beside it.  dict(comps, mesh, casts (CASE_DTYPE: b the cast, vb its delta), ...); bodies rest."""
    o, s = LADDER[rung]
    base = sweep_base()
    body = base["a"]["kind"] != TRIANGLE
    bcases, tcases = base[body], base[~body]
    stride_b, stride_t = -(-len(bcases) // MAX_BODIES), -(-len(tcases) // CC.SMALL_MESH)
    which = WORLD_RUNGS.index(rung) if rung in WORLD_RUNGS else 0
    bcases, tcases = bcases[which % stride_b::stride_b], tcases[which % stride_t::stride_t]
    cases = plant(np.concatenate([bcases, tcases]), rung)
    nb, nf = len(bcases), len(tcases)
    w = dict(comps=CC._comp(cases["a"][:nb]), obstacle=None, compound=None, offset=o, size=s, rung=rung, name="sweeps",
             mesh=dict(verts=cases["a"]["v"][nb:, :9].reshape(3 * nf, 3).astype(np.float32), faces=np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3),
                       pos=np.zeros(3, np.float32)))
    rng = np.random.default_rng(seed + rung)
    c, r = comp_boxes(w["comps"])
    w["aim"] = c.astype(np.float64)
    G = world_grid(w)
    h = float(G["h"])
    lo, hi = G["lo"].astype(np.float64), G["lo"].astype(np.float64) + G["dims"] * h
    extra = []

    def cast(family, tag, p, d, rad, delta):
        n = len(p)
        B = _shape(SPHERE, p, rad) if tag == 0 else _shape(CAPSULE, p, d, rad)
        none = np.zeros(n, SHAPE_DTYPE)     # (no target of its own: the world's are)
        none["kind"] = TRIANGLE
        return CC._cases(family, none, B, None, delta)
    n = 8
    t = w["aim"][rng.integers(0, len(w["aim"]), n)]
    u = _unit(rng, n)
    for mult, nm in ((0.8, "wider_than_a_cell"), (1.7, "wider_than_two_cells")):
        extra.append(cast(f"walk_cast_{nm}", 0, t + u * h * 4.0, None, np.full(n, mult * h), -u * h * 5.0))
        extra.append(cast(f"walk_cast_{nm}", 1, t + u * h * 4.0, _perp(rng, u) * mult * h, np.full(n, 0.4 * mult * h), -u * h * 5.0))
    span = float((hi - lo).min())
    mid = 0.5 * (lo + hi)
    extra.append(cast("walk_cast_wide_as_the_grid", 0, np.tile(mid + [0, span * 2.5, 0], (2, 1)), None, np.full(2, span * 0.55), np.tile([0, -span * 2.0, 0], (2, 1))))
    # a centre path wholly outside the grid whose extent reaches in
    p = np.stack([rng.uniform(lo[0], hi[0], n), np.full(n, hi[1] + 0.9 * h), rng.uniform(lo[2], hi[2], n)], 1)
    extra.append(cast("walk_cast_path_outside_reaches_in", 0, p, None, np.full(n, 1.2 * h), np.tile([h * 3.0, 0, 0], (n, 1))))
    # a best contact in the slab a step brings in: a long cast past bodies that lie ahead and aside
    extra.append(cast("walk_cast_long", 0, t - u * h * 6.0 + _perp(rng, u) * 0.5 * s, None, np.full(n, 0.45 * s), u * h * 12.0))
    extra.append(cast("walk_cast_long", 1, t - u * h * 6.0, _perp(rng, u) * 0.8 * s, np.full(n, 0.3 * s), u * h * 12.0))
    # a capsule whose max(1, |d|) reach at a face is what finds the face: at rest or slow, up to that far from a face of the mesh
    if nf:
        fc = w["mesh"]["verts"].reshape(nf, 3, 3).astype(np.float64).mean(axis=1)[rng.integers(0, nf, n)]
        un = _unit(rng, n)
        ln = np.where(np.arange(n) % 2 == 0, 0.5, 3.0)[:, None]
        extra.append(cast("walk_capsule_reach_at_a_face", 1, fc + un * ln * rng.uniform(0.3, 0.95, (n, 1)), un * ln, np.full(n, 0.05 * s), un * 1e-3))
    w["casts"] = np.concatenate([cases] + extra)
    w["families"] = np.array(CC.FAMILIES)[w["casts"]["family"]]
    return w


def world_casts(w, moving_dtype):
    c = w["casts"]
    out = np.zeros(len(c), moving_dtype)
    comp = CC._comp(c["b"])
    out["tag"], out["p"], out["d"], out["r"], out["delta"] = comp["tag"], comp["p"], comp["d"], comp["r"], c["vb"]
    return out


# ---- the same formulas in float64, and the scan that measured the direction band ------------------------------------------------------------
def _quad_f64(b, a, c, dt):
    """the closing lines of ray_sphere / the end caps: discr, t = max((-b - sqrt(discr)) / a, 0), t <= dt -> (hit, t)"""
    with np.errstate(all="ignore"):
        discr = b * b - a * c
        t = np.fmax((-b - np.sqrt(discr)) / a, 0.0)
        hit = ~((c > 0) & (b > 0)) & ~(discr < 0) & ~(t > dt)
    return hit, t


def answers_f64(cases):
    """hit (n,) bool of mgf_collision.hpp's ray tests evaluated in float64 on the cases' f32 inputs: the same formulas, branches and
    epsilon (ray_sphere :51-62, ray_capsule :65-112, ray_plane / ray_polygon / contains :115-129, :35-42)"""
    p, d, dt = origin(cases).astype(np.float64), cases["vb"].astype(np.float64), cases["dt"].astype(np.float64)
    v = cases["a"]["v"].astype(np.float64)
    kind = cases["a"]["kind"]
    dot = lambda x, y: np.einsum("ij,ij->i", x, y)
    out = np.zeros(len(cases), bool)
    with np.errstate(all="ignore"):
        m = p - v[:, :3]
        nn, mn = dot(d, d), dot(m, d)
        hs, _ = _quad_f64(mn, nn, dot(m, m) - v[:, 3] ** 2, dt)
        out = np.where(kind == SPHERE, hs, out)
        cd, r = v[:, 3:6], v[:, 6]
        md, nd, dd = dot(m, cd), dot(d, cd), dot(cd, cd)
        a, k = dd * nn - nd * nd, dot(m, m) - r * r
        m2 = p - (v[:, :3] + cd)
        ha, ta = _quad_f64(mn, nn, k, dt)
        hb, tb = _quad_f64(dot(m2, d), nn, dot(m2, m2) - r * r, dt)
        par = np.where(md < 0, ha, np.where(md > dd, hb, False))
        c, b = dd * k - md * md, dd * mn - nd * md
        discr = b * b - a * c
        t = (-b - np.sqrt(discr)) / a
        s = md + t * nd
        gen = ~(discr < 0) & ~(t < 0) & np.where(s < 0, ha, np.where(s > dd, hb, ~(t > dt)))
        out = np.where(kind == CAPSULE, np.where(np.abs(a) < 1e-6, par, gen), out)
        A, B, C_ = v[:, :3], v[:, 3:6], v[:, 6:9]
        n = np.cross(B - A, C_ - A)
        n = n / np.sqrt(dot(n, n))[:, None]
        denom = dot(n, d)
        t = (dot(n, A) - dot(n, p)) / denom
        ip = p + d * t[:, None]
        w, ac, ab = ip - A, C_ - A, B - A
        d1, d2, d3, d4, d5 = dot(ac, ac), dot(ac, ab), dot(ac, w), dot(ab, ab), dot(ab, w)
        inv = 1.0 / (d1 * d4 - d2 * d2)
        uu, vv = (d4 * d3 - d2 * d5) * inv, (d1 * d5 - d2 * d3) * inv
        ht = ~(denom == 0) & ~((t <= 0) | (t > dt)) & (uu >= 0) & (vv >= 0) & (uu + vv < 1)
        out = np.where(kind == TRIANGLE, ht, out)
    return out


def band_scan(rungs=WORLD_RUNGS, seed=51, n=40):
    """Per decade of max|d_k| (every decade from 1e-24 to 1e30), over targets as the corpus's worlds hold them at every rung (spheres,
    capsules and triangles of the rung's size and offset, origins within a site's reach and a lattice away), two classes of particle:
    aimed through the middle of the target, and aimed past it by more than twice its bounding sphere - no line of the second class
    comes near its target, so every f32 hit there is a hit that is no hit in float64 (answers_f64 confirms it: the column counts
    f32 hits that float64 denies).  Returns {decade: (through: f32 hits, through: float64 hits, past: f32 hits that float64 denies,
    hits of either class whose t or point is not finite)}.
    (Among the particles aimed through the middle a handful differ between f32 and float64 at every decade alike - a capsule's choice
    between cylinder and end cap, a triangle 0.1 wide whose vertices round by 0.008 at 1e5: local disagreements of rounding, which
    no band of directions removes; the band is about the hits nowhere near the line.)"""
    out = {}
    rng = np.random.default_rng(seed)
    for e in range(-24, 31):
        tot = np.zeros(4, np.int64)
        for rung in rungs:
            o, s = LADDER[rung]
            S = _shape(SPHERE, rng.uniform(-2, 2, (n, 3)), rng.uniform(0.3, 1.2, n))
            K = _capsules(rng, n)
            T = _random_triangles(rng, n)
            for tgt in (S, K, T):
                v = tgt["v"].astype(np.float64)
                kind = tgt["kind"][0]
                ctr = (v[:, :3] + v[:, 3:6] + v[:, 6:9]) / 3.0 if kind == TRIANGLE else v[:, :3] + (0.5 * v[:, 3:6] if kind == CAPSULE else 0.0)
                for reach in (rng.uniform(1.5, 6.0, (n, 1)), rng.uniform(2.0, 8.0, (n, 1)) * PITCH):
                    u = _unit(rng, n)
                    for past in (False, True):          # the bounding spheres have radii below 2
                        aim = ctr + _perp(rng, u) * (6.0 if past else 0.1)
                        p = ctr + u * np.maximum(reach, 12.0 if past else 0.0)
                        dirn = aim - p
                        dirn *= 10.0 ** e / np.abs(dirn).max(axis=1, keepdims=True)
                        c = place(rays("band_scan", tgt, p, dirn), _unit(rng, n) * o, s)
                        c["vb"] = (c["vb"].astype(np.float64) / s).astype(np.float32)      # (the decade is of d itself, not of the rung's scale)
                        hit, ip, t = oracle_answers(c)
                        h, h64 = hit == 1, answers_f64(c)
                        bad = int((h & ~(np.isfinite(t) & np.all(np.isfinite(ip), axis=1))).sum())
                        tot += (0, 0, int((h & ~h64).sum()), bad) if past else (int(h.sum()), int(h64.sum()), 0, bad)
        out[e] = tuple(int(x) for x in tot)
    return out


def band_of(scan):
    """the widest run of decades around 1e0 without a false or non-finite hit, each end pulled in by one decade: (lo, hi) exponents"""
    lo = hi = 0
    while lo - 1 in scan and scan[lo - 1][2:] == (0, 0):
        lo -= 1
    while hi + 1 in scan and scan[hi + 1][2:] == (0, 0):
        hi += 1
    return lo + 1, hi - 1


if __name__ == "__main__":   # python -m tests.query_corpus: the scan of the direction band (EXPERIMENTS.md)
    scan = band_scan()
    print(f"{'max|d_k|':>9s} {'through: f32 hits':>18s} {'f64 hits':>9s} {'past: false hits':>17s} {'not finite':>11s}")
    for e, (h, h64, bad, nf) in scan.items():
        print(f"{'1e%+d' % e:>9s} {h:18d} {h64:9d} {bad:17d} {nf:11d}")
    print("band, each end pulled in by a decade: 1e%+d .. 1e%+d" % band_of(scan))
