"""A seeded corpus of pair-level contact problems with a stated purpose: every branch of the reference's contact tests
(oracle/mgf_collision.hpp, restated for the device in mgf_amd/csrc/dev_geom.h) is the aim of a named family here, and
tests/test_contact_corpus.py measures with gcov that the corpus really reaches them.  Three parts:

  bulk      random shapes and velocities over a scale ladder (centre offsets 0 .. 1e5, sizes x0.05, x1, x20);
  families  constructed cases, each aimed at a branch (the line numbers in the comments are mgf_collision.hpp's);
  reject    cases at the edge of reach of the conservative rejects (comp_pair_far, comp_tri_far) over the same ladder.

A case is a row of CASE_DTYPE: receiver `a` and argument `b` as the oracle's o_shape (kind + 12 floats), their velocities and
the has_vel flags of contacts_batch.  The six types the tick uses: sphere-sphere, capsule-sphere, sphere-capsule,
capsule-capsule (both moving, collision.rs:1387) and triangle-sphere, triangle-capsule (static receiver).

Stated bounds on the inputs (everything else is fair game): coordinates up to 1e5 + a few sizes, radii from 0.002 to 24, axes up to 200 long.
Zero radii appear only in the family "cc_zero_radii" (single-shot only: a world refuses such bodies); the one capsule 1e5 long is the
family "cc_second_sweep_parallel_by_rounding".
"""
import numpy as np

SPHERE, CAPSULE, TRIANGLE = 0, 1, 2
TYPES = ["sphere-sphere", "capsule-sphere", "sphere-capsule", "capsule-capsule", "triangle-sphere", "triangle-capsule"]
_KINDS = {"sphere-sphere": (SPHERE, SPHERE), "capsule-sphere": (CAPSULE, SPHERE), "sphere-capsule": (SPHERE, CAPSULE),
          "capsule-capsule": (CAPSULE, CAPSULE), "triangle-sphere": (TRIANGLE, SPHERE), "triangle-capsule": (TRIANGLE, CAPSULE)}
PAIR_TYPES, TRI_TYPES = TYPES[:4], TYPES[4:]

from oracle.oracle import COMPONENT_DTYPE, SHAPE_DTYPE

CASE_DTYPE = np.dtype([("family", "<i4"), ("rung", "<i4"), ("a", SHAPE_DTYPE), ("b", SHAPE_DTYPE), ("va", "<f4", 3), ("vb", "<f4", 3),
                       ("hv", "u1")])

OFFSETS = [0.0, 1e2, 1e3, 1e4, 1e5]
SIZES = [1.0, 0.05, 20.0]
LADDER = [(o, s) for o in OFFSETS for s in SIZES]   # rung index = position in this list; rung 0 is the plain one

FAMILIES = []          # names; CASE_DTYPE.family indexes this list


def _fam(name):
    if name not in FAMILIES:
        FAMILIES.append(name)
    return FAMILIES.index(name)


def case_type(cases):
    """index into TYPES per case"""
    ka, kb = cases["a"]["kind"], cases["b"]["kind"]
    return np.where(ka == TRIANGLE, 4 + kb, 2 * kb + ka).astype(np.int32)


# ---- building blocks ---------------------------------------------------------------------------------------------------
def _shape(kind, *parts):
    """(n,) SHAPE_DTYPE from float64 column blocks: sphere (c, r), capsule (a, d, r), triangle (a, b, c)"""
    cols = np.concatenate([np.asarray(p, np.float64).reshape(len(parts[0]), -1) for p in parts], axis=1)
    out = np.zeros(len(cols), SHAPE_DTYPE)
    out["kind"] = kind
    out["v"][:, :cols.shape[1]] = cols.astype(np.float32)
    return out


def _cases(family, a, b, va, vb):
    n = len(a)
    out = np.zeros(n, CASE_DTYPE)
    out["family"] = _fam(family)
    out["a"], out["b"] = a, b
    out["vb"] = np.asarray(vb, np.float64).reshape(n, 3).astype(np.float32)
    if a["kind"][0] == TRIANGLE:
        out["hv"] = 2
    else:
        out["va"] = np.asarray(va, np.float64).reshape(n, 3).astype(np.float32)
        out["hv"] = 3
    return out


_POS = {SPHERE: [(0, 3)], CAPSULE: [(0, 3)], TRIANGLE: [(0, 3), (3, 6), (6, 9)]}   # columns that hold points


def place(cases, offset, size):
    """the same cases with every length multiplied by `size` and every point moved by the vector `offset` (n, 3) or (3,), computed in
    f64 and rounded to f32 once.  Axis-aligned directions stay axis-aligned, so exact parallelism survives."""
    out = cases.copy()
    off = np.broadcast_to(np.asarray(offset, np.float64), (len(cases), 3))
    for f in ("a", "b"):
        v = cases[f]["v"].astype(np.float64)
        w = v * size
        for kind in (SPHERE, CAPSULE, TRIANGLE):
            m = cases[f]["kind"] == kind
            for lo, hi in _POS[kind]:
                w[m, lo:hi] = v[m, lo:hi] * size + off[m]
        out[f]["v"] = w.astype(np.float32)
    out["va"] = (cases["va"].astype(np.float64) * size).astype(np.float32)
    out["vb"] = (cases["vb"].astype(np.float64) * size).astype(np.float32)
    return out


def roll_axes(cases, k):
    """the same cases with the coordinate axes renamed cyclically, k[i] steps for case i (an exact operation): the floor families are built
    over the plane y = const, this gives them the two other axis planes - and quat_from_arc(n, z) its identity and half-turn branches"""
    out = cases.copy()
    k = np.broadcast_to(np.asarray(k), (len(cases),))
    for step in (1, 2):
        m = k == step
        for f in ("a", "b"):
            v = out[f]["v"]
            for lo in (0, 3, 6):
                keep = m & ((out[f]["kind"] == TRIANGLE) | (lo == 0) | ((out[f]["kind"] == CAPSULE) & (lo == 3)))
                v[keep, lo:lo + 3] = np.roll(v[keep, lo:lo + 3], step, axis=1)
        for f in ("va", "vb"):
            out[f][m] = np.roll(out[f][m], step, axis=1)
    return out


def over_ladder(cases, rng, rungs=None):
    """`cases` repeated at every rung of the ladder, each case with its own random direction of offset"""
    parts = []
    for k, (o, s) in enumerate(LADDER):
        if rungs is not None and k not in rungs:
            continue
        u = rng.normal(size=(len(cases), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        p = place(cases, u * o, s)
        p["rung"] = k
        parts.append(p)
    return np.concatenate(parts)


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _perp(rng, u):
    w = np.cross(u, rng.normal(size=u.shape))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _rand_shape(rng, kind, n):
    c = rng.uniform(-2, 2, (n, 3))
    if kind == SPHERE:
        return _shape(SPHERE, c, rng.uniform(0.3, 1.2, n))
    if kind == CAPSULE:
        return _shape(CAPSULE, c, rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(0.3, 0.9, n))
    return _shape(TRIANGLE, c, rng.uniform(-2, 2, (n, 3)), rng.uniform(-2, 2, (n, 3)))


# ---- bulk ---------------------------------------------------------------------------------------------------------------
def bulk(seed=1, per_rung=300):
    """random shapes and velocities as tests/test_gpu_parity.py draws them, at every rung"""
    rng = np.random.default_rng(seed)
    parts = []
    for t in TYPES:
        ka, kb = _KINDS[t]
        base = _cases("bulk", _rand_shape(rng, ka, per_rung), _rand_shape(rng, kb, per_rung), rng.uniform(-1, 1, (per_rung, 3)),
                      rng.uniform(-1.5, 1.5, (per_rung, 3)))
        parts.append(over_ladder(base, rng))
    return np.concatenate(parts)


# ---- constructed pair families --------------------------------------------------------------------------------------------
def _axis_point(rng, shape, s):
    """the point at parameter s of the receiver's axis (a sphere: its centre) and a unit vector perpendicular to the axis"""
    v = shape["v"].astype(np.float64)
    if shape["kind"][0] == SPHERE:
        return v[:, :3], _unit(rng, len(v))
    d = v[:, 3:6]
    return v[:, :3] + d * s[:, None], _perp(rng, d / np.linalg.norm(d, axis=1, keepdims=True))


def _arg_at(rng, kind, q, u, r):
    """an argument shape whose axis point nearest to the receiver is q (a capsule: its start, axis leaning away along u)"""
    n = len(q)
    if kind == SPHERE:
        return _shape(SPHERE, q, r)
    d = _unit(rng, n) * rng.uniform(0.3, 1.5, (n, 1))
    d += u * (np.abs(np.einsum("ij,ij->i", d, u)) - np.einsum("ij,ij->i", d, u) + rng.uniform(0.0, 0.5, n))[:, None]
    return _shape(CAPSULE, q, d, r)


def _radius(shape):
    return shape["v"][:, 3 if shape["kind"][0] == SPHERE else 6].astype(np.float64)


def pair_families(t, seed=2, n=60):
    """the constructed families of a pair type: the receiver A random, the argument B placed at a chosen distance from a point of A's axis
    along a perpendicular u, moving along -u so that the surfaces meet at a chosen time"""
    rng = np.random.default_rng(seed + TYPES.index(t))
    ka, kb = _KINDS[t]
    out = []

    def make(family, gap_fn, time_fn, side=0.0, zero_rel=False, n=n):
        A = _rand_shape(rng, ka, n)
        p, u = _axis_point(rng, A, rng.uniform(0.2, 0.8, n))
        rb = rng.uniform(0.3, 0.9, n)
        rsum = _radius(A) + rb.astype(np.float32).astype(np.float64)
        gap = gap_fn(rsum, n)                       # distance of the surfaces (negative: overlap)
        tt = time_fn(n)                             # when the surfaces meet; inf: never (no closing motion)
        w = _perp(rng, u)
        B = _arg_at(rng, kb, p + u * (rsum + gap)[:, None], u, rb)
        with np.errstate(divide="ignore", invalid="ignore"):
            speed = np.where(np.isfinite(tt), np.maximum(gap, 0.0) / tt, 0.0)
        vrel = -u * speed[:, None] + w * side * rng.uniform(-1.0, 1.0, (n, 1))
        va = np.zeros((n, 3)) if not zero_rel else rng.uniform(-1, 1, (n, 3))
        vb = vrel if not zero_rel else va
        # (half of them with the receiver moving as well: collision.rs:1387 subtracts the velocities in f32)
        split = (rng.random(n) < 0.5) & (not zero_rel)
        share = rng.uniform(-0.5, 0.5, (n, 3)) * split[:, None]
        out.append(_cases(family, A, B, va + share, vb + share))

    U = lambda lo, hi: (lambda n_: rng.uniform(lo, hi, n_))
    make("overlap_t0", lambda rs, n_: -rs * rng.uniform(0.05, 0.8, n_), U(0.1, 2.0))
    make("impact_mid", lambda rs, n_: rng.uniform(0.05, 1.0, n_), U(0.05, 0.95))
    make("impact_just_before_1", lambda rs, n_: rng.uniform(0.05, 1.0, n_), U(0.97, 0.9999))
    make("impact_just_after_1", lambda rs, n_: rng.uniform(0.05, 1.0, n_), U(1.0001, 1.05))
    make("tangent_ulps", lambda rs, n_: rs * rng.integers(-4, 5, n_) * 2.0 ** -23, lambda n_: np.full(n_, np.inf))
    make("grazing_ulps", lambda rs, n_: rs * rng.integers(-4, 5, n_) * 2.0 ** -23, lambda n_: np.full(n_, np.inf), side=1.0)
    make("zero_relative_velocity", lambda rs, n_: rs * rng.uniform(-0.6, 0.6, n_), lambda n_: np.full(n_, np.inf), zero_rel=True)
    make("apart_at_rest", lambda rs, n_: rng.uniform(0.01, 1.0, n_), lambda n_: np.full(n_, np.inf))

    # coincident centres / closest points (:501-503, :537-539): coordinates on a grid of quarters, so the points coincide exactly
    def quarters(lo, hi, shape):
        return rng.integers(int(lo * 4), int(hi * 4) + 1, shape) / 4.0
    m = n
    ca = quarters(-2, 2, (m, 3))
    da = quarters(-2, 2, (m, 3)) * 2.0
    da[np.all(da == 0, axis=1)] = (1.0, 0.0, 0.0)
    db = quarters(-2, 2, (m, 3)) * 2.0
    db[np.all(db == 0, axis=1)] = (0.0, 1.0, 0.0)
    ra, rb = rng.uniform(0.3, 0.9, m), rng.uniform(0.3, 0.9, m)
    mid = ca + 0.5 * da                                              # exact: da is a multiple of a half
    A = _shape(SPHERE, mid, ra) if ka == SPHERE else _shape(CAPSULE, ca, da, ra)
    B = _shape(SPHERE, mid, rb) if kb == SPHERE else _shape(CAPSULE, mid - 0.5 * db, db, rb)
    if ka == SPHERE and kb == CAPSULE:                               # the sphere's centre on the capsule's axis
        B = _shape(CAPSULE, mid - 0.5 * db, db, rb)
    v = quarters(-1, 1, (m, 3))
    v[np.all(v == 0, axis=1)] = (0.25, 0.0, 0.0)
    z = np.zeros((m, 3))
    out.append(_cases("coincident_at_rest", A, B, z, z))
    out.append(_cases("coincident_moving", A, B, z, v))
    out.append(_cases("coincident_same_velocity", A, B, v, v))
    return np.concatenate(out)


def capsule_capsule_families(seed=3, n=40):
    """every exit of the parallel branch (:590-641) at rest and moving, with crossing and skew pairs beside them.  The receiver lies along x;
    lengths and positions are multiples of a quarter so that `denom == 0` (geom.rs closest_pts_seg) holds exactly."""
    rng = np.random.default_rng(seed)
    out = []
    q = lambda lo, hi, shape=None: rng.integers(int(lo * 4), int(hi * 4) + 1, shape) / 4.0
    axes = np.eye(3)
    for name, sign in (("parallel", 1.0), ("antiparallel", -1.0)):
        for moving in ("rest", "moving", "along_axis"):
            for rng_case in ("overlapping", "before", "after", "abutting_before", "abutting_after"):
                m = n
                ax = axes[rng.integers(0, 3, m)]
                up = np.roll(ax, 1, axis=1)
                side = np.roll(ax, 2, axis=1)
                la, lb = q(0.5, 3, m), q(0.5, 3, m)
                ra, rb = rng.uniform(0.3, 0.9, m), rng.uniform(0.3, 0.9, m)
                a0 = q(-2, 2, (m, 3))
                # (abutting: the ranges share exactly one end, so that t_max == 0 or t_min == 1 holds with equality, :601-602, :626-627)
                lo = {"overlapping": rng.uniform(-0.9, 0.9, m) * la, "before": -lb - q(0.25, 2, m), "after": la + q(0.25, 2, m),
                      "abutting_before": -lb, "abutting_after": la}[rng_case]
                lo = np.round(lo * 4) / 4
                h = rng.choice([0.0, 0.5, 1.0, 1.75, 2.5], m) * rng.choice([-1.0, 1.0], m)
                b0 = a0 + ax * lo[:, None] + up * h[:, None]
                bd = ax * (lb * sign)[:, None]
                if sign < 0:
                    b0 = b0 + ax * lb[:, None]
                if moving == "rest":
                    v = np.zeros((m, 3))
                elif moving == "along_axis":
                    v = ax * q(-3, 3, m)[:, None]
                else:
                    v = -up * (np.sign(h) * rng.uniform(0.2, 3.0, m))[:, None] + ax * rng.uniform(-2, 2, (m, 1)) * (rng.random((m, 1)) < 0.6) \
                        + side * rng.uniform(-0.3, 0.3, (m, 1)) * (rng.random((m, 1)) < 0.3)
                out.append(_cases(f"cc_{name}_{moving}_{rng_case}", _shape(CAPSULE, a0, ax * la[:, None], ra), _shape(CAPSULE, b0, bd, rb),
                                  np.zeros((m, 3)), v))
    # collinear (h = 0 exactly) is in the draw above (h = 0); crossing and skew: axes along two different coordinate axes
    for name, gap in (("cc_crossing", 0.0), ("cc_skew", 1.0)):
        m = n
        i = rng.integers(0, 3, m)
        ax, bx, up = axes[i], axes[(i + 1) % 3], axes[(i + 2) % 3]
        la, lb = q(0.5, 3, m), q(0.5, 3, m)
        a0 = q(-2, 2, (m, 3))
        h = gap * rng.choice([0.5, 1.0, 1.5, 2.0], m)
        b0 = a0 + ax * (la * 0.5)[:, None] - bx * (lb * 0.5)[:, None] + up * h[:, None]
        for mv, v in (("rest", np.zeros((m, 3))), ("moving", -up * rng.uniform(0.1, 2.5, (m, 1)) + ax * rng.uniform(-1, 1, (m, 1)))):
            out.append(_cases(f"{name}_{mv}", _shape(CAPSULE, a0, ax * la[:, None], rng.uniform(0.3, 0.9, m)),
                              _shape(CAPSULE, b0, bx * lb[:, None], rng.uniform(0.3, 0.9, m)), np.zeros((m, 3)), v))
    # :576 - the first sweep segment not parallel to the receiver, the second parallel: only rounding does that (v.y is lost at y = 1e5)
    m = 8
    a0 = np.zeros((m, 3))
    b0 = np.stack([q(-1, 1, m), np.full(m, 1.0), np.zeros(m)], 1)
    out.append(_cases("cc_second_sweep_parallel_by_rounding", _shape(CAPSULE, a0, np.tile([2.0, 0, 0], (m, 1)), np.full(m, 0.5)),
                      _shape(CAPSULE, b0, np.tile([0, 1e5, 0], (m, 1)), np.full(m, 0.5)), np.zeros((m, 3)), np.tile([1.0, 1e-3, 0.0], (m, 1))))
    return np.concatenate(out)


def capsule_capsule_zero_radii(seed=4, n=8):
    """:634-636 - is_zero(ab) after the travel to first touch: the axis points coincide when the surfaces touch, i.e. the radii sum to zero"""
    rng = np.random.default_rng(seed)
    la = rng.integers(2, 12, n) / 4.0
    h = rng.integers(1, 8, n) / 4.0
    a0 = rng.integers(-8, 8, (n, 3)) / 4.0
    ax, up = np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    A = _shape(CAPSULE, a0, ax * la[:, None], np.zeros(n))
    B = _shape(CAPSULE, a0 + up * h[:, None], ax * la[:, None], np.zeros(n))
    return _cases("cc_zero_radii", A, B, np.zeros((n, 3)), -up * (2.0 * h)[:, None])


# ---- triangles ----------------------------------------------------------------------------------------------------------------
def _rand_tris(rng, n):
    """well-shaped triangles: an equilateral one of side 1.5 .. 3, turned any way and nudged"""
    c = rng.uniform(-2, 2, (n, 3))
    u = _unit(rng, n)
    w = _perp(rng, u)
    s = rng.uniform(1.5, 3.0, (n, 1))
    a = c + u * s * 0.577
    b = c + (-0.5 * u + 0.866 * w) * s * 0.577
    cc = c + (-0.5 * u - 0.866 * w) * s * 0.577
    return a + rng.normal(0, 0.1, (n, 3)), b + rng.normal(0, 0.1, (n, 3)), cc + rng.normal(0, 0.1, (n, 3))


def _tri_normal(a, b, c):
    nn = np.cross(b - a, c - a)
    return nn / np.linalg.norm(nn, axis=1, keepdims=True)


def _tri_targets(rng, a, b, c, where):
    """a point of the triangle's plane: inside the face, a little outside an edge, or a little outside a vertex"""
    n = len(a)
    ctr = (a + b + c) / 3.0
    V = [a, b, c]
    if where == "face":
        w = rng.dirichlet((2.0, 2.0, 2.0), n)
        return w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c, np.zeros((n, 3))
    if where.startswith("edge"):
        i = int(where[-1])
        p0, p1 = V[i], V[(i + 1) % 3]
        on = p0 + (p1 - p0) * rng.uniform(0.15, 0.85, (n, 1))
    else:
        on = V[int(where[-1])]
    outward = on - ctr
    outward -= _tri_normal(a, b, c) * np.einsum("ij,ij->i", outward, _tri_normal(a, b, c))[:, None]
    return on, outward / np.linalg.norm(outward, axis=1, keepdims=True)


def triangle_sphere_families(seed=5, n=40):
    rng = np.random.default_rng(seed)
    out = []
    for where in ("face", "edge0", "edge1", "edge2", "vertex0", "vertex1", "vertex2"):
        for side, sname in ((1.0, "front"), (-1.0, "back")):
            for motion in ("overlap", "impact", "late", "rest", "miss"):
                a, b, c = _rand_tris(rng, n)
                nrm = _tri_normal(a, b, c) * side
                on, outward = _tri_targets(rng, a, b, c, where)
                r = rng.uniform(0.3, 0.9, n)
                off = outward * (r * rng.uniform(0.0, 0.7, n))[:, None]
                g = {"overlap": -r * rng.uniform(0.1, 0.9, n), "rest": rng.uniform(-0.3, 0.5, n) * r}.get(motion, rng.uniform(0.05, 1.0, n))
                tt = {"overlap": rng.uniform(0.2, 2.0, n), "impact": rng.uniform(0.05, 0.95, n), "late": rng.uniform(1.0001, 1.1, n),
                      "rest": np.full(n, np.inf), "miss": rng.uniform(0.1, 0.9, n)}[motion]
                centre = on + off + nrm * (r + g)[:, None]
                v = -nrm * (np.maximum(g, 0.05) / tt)[:, None] - outward * (np.maximum(g, 0.05) / tt * rng.uniform(0.0, 0.6, n))[:, None]
                if motion == "miss":
                    v = -v
                if motion == "rest":
                    v = np.zeros((n, 3))
                out.append(_cases(f"ts_{where}_{sname}_{motion}", _shape(TRIANGLE, a, b, c), _shape(SPHERE, centre, r), None, v))
    return np.concatenate(out)


def _floor_tris(rng, n, rot):
    """right triangles in the plane y = y0 with two edges along x and z; `rot` turns the vertex order so that the axis-aligned edges take
    every edge index in turn.  Quarter-grid coordinates."""
    q = lambda lo, hi, shape=None: rng.integers(int(lo * 4), int(hi * 4) + 1, shape) / 4.0
    o = q(-2, 2, (n, 3))
    sx, sz = q(1.5, 4, n), q(1.5, 4, n)
    flip = rng.choice([-1.0, 1.0], (n, 2))
    V = [o, o + np.stack([sx * flip[:, 0], np.zeros(n), np.zeros(n)], 1), o + np.stack([np.zeros(n), np.zeros(n), sz * flip[:, 1]], 1)]
    return V[rot % 3], V[(rot + 1) % 3], V[(rot + 2) % 3], o, sx * flip[:, 0], sz * flip[:, 1]


def triangle_capsule_families(seed=6, n=40):
    rng = np.random.default_rng(seed)
    out = []
    q = lambda lo, hi, shape=None: rng.integers(int(lo * 4), int(hi * 4) + 1, shape) / 4.0
    # -- the axis crosses the face (:280-291), from either side, at rest and moving
    a, b, c = _rand_tris(rng, n)
    nrm = _tri_normal(a, b, c)
    on, _ = _tri_targets(rng, a, b, c, "face")
    h1, h2 = rng.uniform(0.1, 1.0, n), rng.uniform(0.1, 1.0, n)
    sgn = rng.choice([-1.0, 1.0], n)
    start = on + nrm * (sgn * h1)[:, None]
    d = -nrm * (sgn * (h1 + h2))[:, None] + _perp(rng, nrm) * rng.uniform(0, 0.3, (n, 1))
    out.append(_cases("tc_axis_crosses_face", _shape(TRIANGLE, a, b, c), _shape(CAPSULE, start, d, rng.uniform(0.2, 0.6, n)), None,
                      rng.uniform(-1, 1, (n, 3)) * (rng.random((n, 1)) < 0.7)))
    # -- a capsule level over a floor triangle (exactly parallel to the face: |dir . n| < eps, :342, :359)
    for rot in range(3):
        for form in ("both_ends_t0", "one_end_t0", "one_end_falling", "silhouette_falling", "beside_falling", "level_random"):
            ta, tb, tc, o, sx, sz = _floor_tris(rng, n, rot)
            r = rng.uniform(0.3, 0.8, n)
            inside = lambda lo=0.1, hi=0.35: o + np.stack([sx * rng.uniform(lo, hi, n), np.zeros(n), sz * rng.uniform(lo, hi, n)], 1)
            beyond = lambda: o + np.stack([sx * rng.uniform(0.8, 1.6, n), np.zeros(n), sz * rng.uniform(0.8, 1.6, n)], 1)
            behind = lambda: o - np.stack([sx * rng.uniform(0.2, 0.8, n), np.zeros(n), sz * rng.uniform(0.2, 0.8, n)], 1)
            up = np.array([0.0, 1.0, 0.0])
            if form == "both_ends_t0":        # two contacts from one face (:306-312)
                p0, p1, hgt, fall = inside(), inside(), r * rng.uniform(0.2, 0.95, n), rng.uniform(0.0, 1.0, n)
            elif form == "one_end_t0":        # :313-316 then the clipped silhouette at t = 0 (:343-357)
                p0, p1, hgt, fall = inside(), beyond(), r * rng.uniform(0.2, 0.95, n), rng.uniform(0.0, 1.0, n)
            elif form == "one_end_falling":   # :321 / :304, then :343-357 with t > 0
                p0, p1, hgt = inside(), beyond(), r + rng.uniform(0.05, 0.8, n)
                fall = (hgt - r) / rng.uniform(0.1, 0.95, n)
            elif form == "silhouette_falling":  # both ends outside, the axis over the face: :359-381
                p0, p1, hgt = behind(), beyond(), r + rng.uniform(0.05, 0.8, n)
                fall = (hgt - r) / rng.uniform(0.1, 0.95, n)
            elif form == "beside_falling":    # both ends outside and the axis beside the face: falls through to the Minkowski part
                p0 = behind()
                p1 = p0 + np.stack([-sx * rng.uniform(0.1, 0.5, n), np.zeros(n), sz * rng.uniform(0.1, 1.0, n)], 1)
                hgt = r + rng.uniform(0.05, 0.8, n)
                fall = (hgt - r) / rng.uniform(0.1, 0.95, n)
            else:
                p0, p1 = inside(-0.5, 1.2), inside(-0.5, 1.2)
                hgt, fall = r * rng.uniform(0.2, 2.5, n), rng.uniform(0.0, 2.0, n)
            swap = rng.random(n) < 0.5          # (either end first: :304 / :316 / :328)
            s0, s1 = np.where(swap[:, None], p1, p0), np.where(swap[:, None], p0, p1)
            start = s0 + up * hgt[:, None]
            dd = (s1 - s0).astype(np.float32).astype(np.float64)
            dd[:, 1] = 0.0
            v = -up * fall[:, None] + np.stack([rng.uniform(-0.3, 0.3, n), np.zeros(n), rng.uniform(-0.3, 0.3, n)], 1) * (rng.random((n, 1)) < 0.5)
            out.append(_cases(f"tc_level_{form}_rot{rot}", _shape(TRIANGLE, ta, tb, tc), _shape(CAPSULE, start, dd, r), None, v))
    # -- exactly parallel to an edge, both directions (:396 holds; both ray_capsule sub-branches :404-419), at random heights and velocities
    for rot in range(3):
        for along in ("x", "z"):
            for sign in (1.0, -1.0):
                m = 2 * n
                ta, tb, tc, o, sx, sz = _floor_tris(rng, m, rot)
                r = rng.uniform(0.2, 0.7, m)
                ln = q(0.5, 3, m)
                e = np.array([1.0, 0, 0]) if along == "x" else np.array([0, 0, 1.0])
                other = np.array([0, 0, 1.0]) if along == "x" else np.array([1.0, 0, 0])
                ext, oth = (sx, sz) if along == "x" else (sz, sx)
                pos = rng.uniform(-1.6, 1.6, m) * np.abs(ext) * np.sign(ext)          # where along the edge's line the capsule starts
                out_d = -np.sign(oth) * rng.uniform(0.0, 1.5, m)                      # outside the face, beyond the edge
                hgt = rng.uniform(-0.5, 1.5, m)
                start = o + e * pos[:, None] + other * out_d[:, None] + np.array([0, 1.0, 0]) * hgt[:, None]
                v = other * (-out_d * rng.uniform(0.0, 2.0, m))[:, None] + np.array([0, 1.0, 0]) * (-hgt * rng.uniform(0.0, 2.0, m))[:, None] \
                    + e * rng.uniform(-1.5, 1.5, (m, 1)) * (rng.random((m, 1)) < 0.5)
                out.append(_cases(f"tc_parallel_edge_{along}{'+' if sign > 0 else '-'}_rot{rot}", _shape(TRIANGLE, ta, tb, tc),
                                  _shape(CAPSULE, start, e * (ln * sign)[:, None], r), None, v))
    # -- edge quads and vertex capsules (:422-472): a capsule outside the face near an edge or a vertex, any direction, closing in
    for where in ("edge0", "edge1", "edge2", "vertex0", "vertex1", "vertex2"):
        a, b, c = _rand_tris(rng, n)
        nrm = _tri_normal(a, b, c)
        on, outward = _tri_targets(rng, a, b, c, where)
        r = rng.uniform(0.2, 0.6, n)
        g = rng.uniform(0.05, 0.8, n)
        away = outward * rng.uniform(0.5, 1.0, (n, 1)) + nrm * rng.uniform(-0.7, 0.7, (n, 1))
        away /= np.linalg.norm(away, axis=1, keepdims=True)
        d = _unit(rng, n) * rng.uniform(0.3, 1.5, (n, 1))
        d += away * (np.abs(np.einsum("ij,ij->i", d, away)) - np.einsum("ij,ij->i", d, away))[:, None]   # leaning away: the start is nearest
        start = on + away * (r + g)[:, None]
        flip = rng.random(n) < 0.5                                                                        # ... or the far end is
        start, d = np.where(flip[:, None], start + d, start), np.where(flip[:, None], -d, d)
        v = -away * (g / rng.uniform(0.1, 1.05, n))[:, None]
        out.append(_cases(f"tc_{where}_closing", _shape(TRIANGLE, a, b, c), _shape(CAPSULE, start, d, r), None, v))
    out = np.concatenate(out)
    floor = np.array([FAMILIES[f].startswith(("tc_level", "tc_parallel_edge")) for f in out["family"]])
    return roll_axes(out, np.where(floor, np.arange(len(out)) % 3, 0))


def degenerate_triangles(seed=7, n=12):
    """collinear or repeated vertices: whatever the oracle answers (NaN included) is the expectation"""
    rng = np.random.default_rng(seed)
    out = []
    for kb in (SPHERE, CAPSULE):
        for kind in ("collinear", "two_equal", "all_equal"):
            a = rng.integers(-8, 8, (n, 3)) / 4.0
            e = rng.integers(-8, 8, (n, 3)) / 4.0
            e[np.all(e == 0, axis=1)] = (1.0, 0, 0)
            b = a + e if kind != "all_equal" else a.copy()
            c = a + 2.0 * e if kind == "collinear" else (a.copy() if kind == "all_equal" else b.copy())
            B = _rand_shape(rng, kb, n)
            B["v"][:, :3] += a.astype(np.float32)
            out.append(_cases(f"degenerate_{kind}", _shape(TRIANGLE, a, b, c), B, None, rng.uniform(-1.5, 1.5, (n, 3)) * (rng.random((n, 1)) < 0.8)))
    return np.concatenate(out)


# ---- reject stress -------------------------------------------------------------------------------------------------------------------
def reject_pairs(seed=8, n=240):
    """the three families of test_pair_contacts_at_the_edge_of_reach (head-on at the end of the sweep, grazing, resting a hair apart), drawn at
    unit scale around the origin and then placed over the ladder - small bodies far from the origin included"""
    rng = np.random.default_rng(seed)
    out = []
    for t in PAIR_TYPES:
        ka, kb = _KINDS[t]
        for mode, name in enumerate(("head_on", "grazing", "resting")):
            ra, rb = rng.uniform(0.2, 0.9, n), rng.uniform(0.2, 0.9, n)
            da = _unit(rng, n) * rng.uniform(0.1, 1.5, (n, 1)) * (ka == CAPSULE)
            db = _unit(rng, n) * rng.uniform(0.1, 1.5, (n, 1)) * (kb == CAPSULE)
            pa = rng.uniform(-2, 2, (n, 3))
            Ra, Rb = ra + 0.5 * np.linalg.norm(da, axis=1), rb + 0.5 * np.linalg.norm(db, axis=1)
            u = _unit(rng, n)
            speed = rng.uniform(0.0, 3.0, n)
            side = np.zeros((n, 3))
            if mode == 0:
                gap = (Ra + Rb + speed) * rng.uniform(0.9, 1.02, n)
            elif mode == 1:
                gap = speed * rng.uniform(0.2, 1.0, n)
                side = _perp(rng, u) * ((ra + rb) * rng.uniform(0.8, 1.05, n))[:, None]
            else:
                speed = rng.uniform(0.0, 1e-3, n)
                gap = (ra + rb) * rng.uniform(0.7, 1.3, n)
            ma = pa + 0.5 * da
            pb = ma + u * gap[:, None] + side - 0.5 * db
            vb = -u * (speed * rng.uniform(0.5, 1.0, n))[:, None]
            va = u * (speed * rng.uniform(0.0, 0.5, n))[:, None]
            A = _shape(SPHERE, pa, ra) if ka == SPHERE else _shape(CAPSULE, pa, da, ra)
            B = _shape(SPHERE, pb, rb) if kb == SPHERE else _shape(CAPSULE, pb, db, rb)
            out.append(_cases(f"reject_{name}", A, B, va, vb))
        # collinear, tip to tip: the distance of the bounding spheres is the sum of their radii and a hair
        ra, rb = rng.uniform(0.4, 1.0, n), rng.uniform(0.4, 1.0, n)
        u = _unit(rng, n)
        la, lb = rng.uniform(0.5, 3.0, n) * (ka == CAPSULE), rng.uniform(0.5, 3.0, n) * (kb == CAPSULE)
        pa = rng.uniform(-2, 2, (n, 3))
        gap = (ra + rb) * rng.uniform(0.98, 1.01, n)
        pb = pa + u * (la + gap)[:, None]
        A = _shape(SPHERE, pa, ra) if ka == SPHERE else _shape(CAPSULE, pa, u * la[:, None], ra)
        B = _shape(SPHERE, pb, rb) if kb == SPHERE else _shape(CAPSULE, pb, u * lb[:, None], rb)
        out.append(_cases("reject_tip_to_tip", A, B, np.zeros((n, 3)), -u * rng.uniform(0.0, 0.05, (n, 1))))
    return over_ladder(np.concatenate(out), np.random.default_rng(seed + 100))


def reject_triangles(seed=9, n=400):
    """the draws of tests/test_gpu_tri_reject.py (bodies at about the reach of a random point of the face; a heightfield's faces with bodies lying
    along its edges) at unit scale, placed over the ladder"""
    rng = np.random.default_rng(seed)
    out = []
    for kb in (SPHERE, CAPSULE):
        for near in (0.6, 1.0, 1.1, 1.6):
            a, b, c = _rand_tris(rng, n)
            thin = rng.random(n) < 0.15
            c[thin] = a[thin] + (b[thin] - a[thin]) * rng.uniform(0, 1, (thin.sum(), 1)) + rng.normal(0, 0.02, (thin.sum(), 3))
            r = rng.uniform(0.05, 1.0, n)
            d = _unit(rng, n) * rng.uniform(0.0, 2.0, (n, 1)) * (kb == CAPSULE)
            w = rng.dirichlet((1.0, 1.0, 1.0), n)
            on = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
            reach = r + np.linalg.norm(d, axis=1)
            p = on + _unit(rng, n) * (reach * rng.uniform(0.0, near, n))[:, None] - 0.5 * d * rng.uniform(0.0, 2.0, (n, 1))
            v = _unit(rng, n) * rng.choice([0.0, 1e-3, 0.05, 0.5, 2.0], (n, 1))
            B = _shape(SPHERE, p, r) if kb == SPHERE else _shape(CAPSULE, p, d, r)
            out.append(_cases("reject_tri_reach", _shape(TRIANGLE, a, b, c), B, None, v))
        # heightfield faces, bodies lying on and beside them, axes along x / z / level / anywhere
        cell = 1.0
        ij = rng.integers(-3, 3, (n, 2)).astype(np.float64)
        h = rng.uniform(-0.2, 0.2, (n, 4)) * (rng.random((n, 1)) < 0.7)
        x0, z0 = ij[:, 0] * cell, ij[:, 1] * cell
        corners = np.stack([np.stack([x0, h[:, 0], z0], 1), np.stack([x0 + cell, h[:, 1], z0], 1),
                            np.stack([x0, h[:, 2], z0 + cell], 1), np.stack([x0 + cell, h[:, 3], z0 + cell], 1)], 1)
        upper = rng.random(n) < 0.5
        tris = np.where(upper[:, None, None], corners[:, [1, 3, 2]], corners[:, [0, 1, 2]])
        r = rng.choice([0.1, 0.25, 0.3, 0.5], n)
        length = rng.choice([0.2, 0.6, 1.0, 1.4, 3.0], n)
        kind = rng.integers(0, 4, n)
        axis = rng.normal(0, 1, (n, 3))
        axis[kind == 0] = (1.0, 0, 0); axis[kind == 1] = (0, 0, 1.0)
        axis[kind == 2, 1] = 0.0
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        d = axis * length[:, None] * (kb == CAPSULE)
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        on = np.einsum("nk,nkj->nj", w, tris)
        side = rng.normal(0, 1, (n, 3)) * np.array([1.0, 0, 1.0]) * rng.choice([0.0, 0.3, 1.0, 2.5], (n, 1)) * cell
        height = r * rng.choice([0.5, 0.98, 1.0, 1.02, 1.5, 3.0], n)
        p = on + side + np.array([0, 1.0, 0]) * height[:, None] - d * rng.uniform(0, 1, (n, 1))
        v = rng.normal(0, 1, (n, 3)) * rng.choice([1e-5, 1e-3, 0.02, 0.2], (n, 1))
        fall = rng.random(n) < 0.5
        v[fall, 0] = 0.0; v[fall, 2] = 0.0
        B = _shape(SPHERE, p, r) if kb == SPHERE else _shape(CAPSULE, p, d, r)
        out.append(_cases("reject_tri_heightfield", _shape(TRIANGLE, tris[:, 0], tris[:, 1], tris[:, 2]), B, None, v))
    return over_ladder(np.concatenate(out), np.random.default_rng(seed + 100))


# ---- the whole corpus --------------------------------------------------------------------------------------------------------------
def families(zero_radii=True):
    """the constructed families at rung 0, and again over the ladder (the exact constructions survive `place`)"""
    rng = np.random.default_rng(10)
    parts = [pair_families(t) for t in PAIR_TYPES] + [capsule_capsule_families(), triangle_sphere_families(), triangle_capsule_families(),
                                                      degenerate_triangles()]
    base = np.concatenate(parts)
    plain = base[base["family"] != _fam("cc_second_sweep_parallel_by_rounding")]      # (that family is about one particular rounding: rung 0 only)
    laddered = over_ladder(plain[::3], rng, rungs=range(1, len(LADDER)))
    out = [base, laddered]
    if zero_radii:
        out.append(capsule_capsule_zero_radii())
    # a capsule whose axis the coordinates hardly resolve, 2.7 degrees off an edge of a face 5 m away: the reference extrudes the edge by the axis,
    # the quad comes out collinear by rounding, and it reports a contact at t = 0 (a world of 32-part bodies found it; comp_tri_far has to let it by)
    far = _cases("reject_tri_unresolved_axis",
                 _shape(TRIANGLE, [[100001.125, 5.9375, 65.48750305175781]], [[100001.125, 6.0625, 65.48750305175781]], [[100001.125, 6.0625, 65.38749694824219]]),
                 _shape(CAPSULE, [[100001.140625, 6.086218, 60.378822]], [[-0.001751183, 5.197018e-07, -0.0366662]], [0.015861]), None,
                 [[6.8896916e-05, -2.3835950e-05, -2.8857214e-06]])
    far["rung"] = 13
    out.append(far)
    return np.concatenate(out)


def corpus(zero_radii=True):
    """bulk + families + reject stress; deterministic"""
    FAMILIES.clear()
    return np.concatenate([bulk(), families(zero_radii), reject_pairs(), reject_triangles()])


# ---- answers --------------------------------------------------------------------------------------------------------------------------
def oracle_answers(cases):
    """(contacts (n, 2) CONTACT_DTYPE, counts (n,)) of the oracle's single-shot entry"""
    from oracle import oracle as O
    return O.contacts_batch(cases["a"], cases["va"], cases["b"], cases["vb"], cases["hv"], slots=2)


def classes(cases, contacts, counts):
    """per type: how many cases have no contact, a contact at t = 0, a contact with 0 < t <= 1, two contacts"""
    ty = case_type(cases)
    t0 = contacts["t"][:, 0]
    out = {}
    for i, name in enumerate(TYPES):
        m = ty == i
        out[name] = dict(none=int((m & (counts == 0)).sum()), t0=int((m & (counts > 0) & (t0 == 0)).sum()),
                         moving=int((m & (counts > 0) & (t0 > 0) & (t0 <= 1)).sum()), two=int((m & (counts == 2)).sum()))
    return out


def same_f32(got, want):
    """the suite's meaning of exact (tests/util.values_equal: +0 == -0), with NaN in the same place counting as equal"""
    return np.array_equal(np.asarray(got, np.float32), np.asarray(want, np.float32), equal_nan=True)


# ---- the world form: cases planted in worlds ------------------------------------------------------------------------------------------
PITCH = 24.0        # lattice pitch at size 1: a case spans at most +-6 around its site and moves at most 4, so cases do not meet
WORLD_RUNGS = [0, 4, 8, 9, 12, 13]   # (0, x1) (1e2, x0.05) (1e3, x20) (1e4, x1) (1e5, x1) (1e5, x0.05)
# families that cannot be planted: a world refuses a zero radius; a capsule 1e5 long meets every case of the lattice
UNPLANTABLE = ("cc_zero_radii", "cc_second_sweep_parallel_by_rounding")


def _comp(shape):
    out = np.zeros(len(shape), COMPONENT_DTYPE)
    cap = shape["kind"] == CAPSULE
    out["tag"] = shape["kind"]
    out["p"] = shape["v"][:, :3]
    out["d"][cap] = shape["v"][cap, 3:6]
    out["r"] = np.where(cap, shape["v"][:, 6], shape["v"][:, 3])
    return out


def base_cases(types, per_family=None, seed=11):
    """the rung-0 cases of the given types that a world can hold (bulk, families and reject stress), optionally thinned to at most
    `per_family` of each family and type"""
    FAMILIES.clear()
    parts = [bulk(per_rung=120), families(zero_radii=False), reject_pairs(n=40), reject_triangles(n=60)]
    c = np.concatenate(parts)
    c = c[c["rung"] == 0]
    names = np.array(FAMILIES)[c["family"]]
    ty = case_type(c)
    keep = ~np.isin(names, UNPLANTABLE) & np.isin(ty, [TYPES.index(t) for t in types])
    c, names, ty = c[keep], names[keep], ty[keep]
    if per_family is not None:
        rng = np.random.default_rng(seed)
        sel = []
        for key in sorted(set(zip(names.tolist(), ty.tolist()))):
            idx = np.nonzero((names == key[0]) & (ty == key[1]))[0]
            sel.append(rng.permutation(idx)[:per_family])
        c = c[np.sort(np.concatenate(sel))]
    return c


def _sites(n, rung, stride=1):
    """the positions of n sites of a cubic lattice whose origin and scale come from the ladder (`stride` sites apart along z for tenants
    that are wider than one site); multiples of the pitch, exact in f32 for the sizes of the ladder up to the rounding `place` does once"""
    o, s = LADDER[rung]
    side = int(np.ceil(n ** (1.0 / 3.0)))
    k = np.arange(n)
    site = np.stack([k % side, (k // side) % side, (k // (side * side)) * stride], 1).astype(np.float64) * PITCH
    return np.array([o, 0.0, 0.0]) + site * s


def plant(cases, rung):
    """the cases laid on the lattice: site k holds case k"""
    out = place(cases, _sites(len(cases), rung), LADDER[rung][1])
    out["rung"] = rung
    return out


def _world(comps, delta, mesh=None, obstacle=None, compound=None, cdelta=None):
    return dict(comps=comps, delta=np.ascontiguousarray(delta, np.float32), mesh=mesh, obstacle=obstacle, compound=compound, cdelta=cdelta)


def pair_world(cases, with_obstacle=False):
    """planted pair cases as bodies: the argument B first, the receiver A behind it - body i's partners are the bodies below it and the pair
    test runs as contacts(i, j) (world.rs:253-285), so A has to be the later one.  with_obstacle: the cases whose receiver does not move
    become one static Compound of their receivers, each argument a body."""
    if with_obstacle:
        cases = cases[np.all(cases["va"] == 0, axis=1)]
        return _world(_comp(cases["b"]), cases["vb"], obstacle=_comp(cases["a"]))
    comps = np.zeros(2 * len(cases), COMPONENT_DTYPE)
    delta = np.zeros((2 * len(cases), 3), np.float32)
    comps[0::2], comps[1::2] = _comp(cases["b"]), _comp(cases["a"])
    delta[0::2], delta[1::2] = cases["vb"], cases["va"]
    return _world(comps, delta)


def with_mesh(world, tri_cases):
    """the world with the planted triangle cases added: every triangle a face of the mesh, every argument one more body"""
    n = len(tri_cases)
    out = dict(world)
    out["comps"] = np.concatenate([world["comps"], _comp(tri_cases["b"])])
    out["delta"] = np.concatenate([world["delta"], tri_cases["vb"]])
    out["mesh"] = dict(verts=tri_cases["a"]["v"][:, :9].reshape(3 * n, 3).astype(np.float32), faces=np.arange(3 * n, dtype=np.uint32).reshape(n, 3),
                       pos=np.zeros(3, np.float32))
    return out


LIVE_PARTS = 12     # part pairs of two many-part bodies that may meet: the HIP path refuses more than 64 raw contacts or a manifold above 16


def parts_world(pairs, tris, parts, rung, spacing=10.0, obstacle=False):
    """bodies of `parts` components drawn from the corpus.  Every case leads one group: the case and the parts - 1 after it (cyclically), laid
    `spacing` apart along z.  A group of pair cases makes a pair of bodies - the arguments one body, the receivers the other (obstacle: the
    receivers of all groups are one static Compound instead) - and a group of triangle cases a body of its arguments over faces of its
    triangles.  A body moves as its leading case's shape does, so the leading case is planted exactly and the others with another motion.
    Beyond LIVE_PARTS members a pair group's receivers stand half a pitch aside: parts of the body that meet nothing."""
    s = LADDER[rung][1]
    if obstacle:
        pairs = pairs[np.all(pairs["va"] == 0, axis=1)]
    sites = _sites(len(pairs) + len(tris), rung, stride=int(np.ceil(parts * spacing / PITCH)) + 1)

    def members(cases, first):
        n = len(cases)
        idx = (np.arange(n)[:, None] + np.arange(parts)[None, :]) % n
        off = sites[first:first + n, None, :] + np.arange(parts)[None, :, None] * np.array([0.0, 0.0, spacing * s])
        return place(cases[idx.ravel()], off.reshape(-1, 3), s)
    P, T = members(pairs, 0), members(tris, len(pairs))
    aside = np.tile(np.arange(parts) >= LIVE_PARTS, len(pairs))
    P["a"]["v"][aside, 1] += np.float32(0.5 * PITCH * s)
    lead_p, lead_t = place(pairs, np.zeros(3), s), place(tris, np.zeros(3), s)
    bodies = [_comp(P["b"])] + ([] if obstacle else [_comp(P["a"])]) + [_comp(T["b"])]
    cdelta = np.concatenate([lead_p["vb"]] + ([] if obstacle else [lead_p["va"]]) + [lead_t["vb"]])
    comps = np.concatenate(bodies)
    w = _world(np.zeros(0, COMPONENT_DTYPE), np.zeros((0, 3), np.float32), obstacle=_comp(P["a"]) if obstacle else None,
               compound=dict(comps=comps, offsets=np.arange(0, len(comps) + 1, parts, dtype=np.int64)), cdelta=cdelta)
    nf = len(T)
    if nf:
        w["mesh"] = dict(verts=T["a"]["v"][:, :9].reshape(3 * nf, 3).astype(np.float32), faces=np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3),
                         pos=np.zeros(3, np.float32))
    return w


SMALL_MESH = 63     # faces: below the 64 from which a world lays a grid over its mesh's faces (the rows of k_integrate's tail serve instead)


def world_scenes(rung):
    """name -> world of the world form at one rung of the ladder (see tests/test_gpu_contact_corpus.py for the front ends each one runs under).
    The worlds with a small mesh take a different slice of the triangle cases at every rung; the *_face_grid worlds hold them all."""
    out = {}
    o, s = LADDER[rung]
    ss = plant(base_cases(["sphere-sphere"]), rung)
    ts = plant(base_cases(["triangle-sphere"], per_family=6), rung)
    mixed = plant(base_cases(PAIR_TYPES[1:]), rung)
    tris = plant(base_cases(TRI_TYPES, per_family=8), rung)

    def some(t, k):
        stride = -(-len(t) // SMALL_MESH)
        return t[(WORLD_RUNGS.index(rung) * 3 + k) % stride::stride] if rung in WORLD_RUNGS else t[k % stride::stride]
    out["spheres"] = with_mesh(pair_world(ss), some(ts, 0))
    out["spheres_face_grid"] = with_mesh(pair_world(ss[::4]), ts)
    for k in range(3):
        out[f"mixed_{k}"] = with_mesh(pair_world(mixed[k::3]), some(tris, k))
    out["mixed_face_grid"] = with_mesh(pair_world(mixed[::4]), tris)
    out["obstacle"] = pair_world(plant(base_cases(PAIR_TYPES), rung), with_obstacle=True)
    # bodies of several parts: 2 (k_pair_grid_n<true>, k_terrain_contacts<2>), 4 (the *_parts<kMaxParts> kernels), 7 and 32 (k_narrow_pairs_big,
    # k_narrow_terrain_big: a lane per part), over a small mesh, over a face grid and beside an obstacle
    pc, tc = base_cases(PAIR_TYPES, per_family=6), base_cases(TRI_TYPES, per_family=4)
    which = WORLD_RUNGS.index(rung) if rung in WORLD_RUNGS else 0

    def few(parts):
        m = SMALL_MESH // parts
        stride = -(-len(tc) // m)
        return tc[which % stride::stride][:m]
    out["two_parts"] = parts_world(pc, few(2), 2, rung)
    out["two_parts_face_grid"] = parts_world(pc[::2], tc, 2, rung)
    out["four_parts"] = parts_world(pc[::2], few(4), 4, rung)
    out["four_parts_face_grid"] = parts_world(pc[::3], tc[::2], 4, rung)
    out["three_parts_obstacle"] = parts_world(pc, tc[:0], 3, rung, obstacle=True)
    out["seven_parts"] = parts_world(pc[::2], tc[::2], 7, rung)
    out["seven_parts_small_mesh"] = parts_world(pc[::3], few(7), 7, rung)
    out["thirty_two_parts"] = parts_world(pc[::5], tc[::4], 32, rung)
    # fast movers whose fat box is far wider than the rest's (ten times the largest motion of a case), through and beside the lattice
    w = pair_world(ss)
    lo, hi = w["comps"]["p"].min(axis=0).astype(np.float64), w["comps"]["p"].max(axis=0).astype(np.float64)
    mid = 0.5 * (lo + hi)
    fast = np.zeros(4, COMPONENT_DTYPE)
    fast["p"] = [mid, lo - 3.0 * s, mid + (0.0, 40.0 * s, 0.0), mid + (0.3 * s, 40.8 * s, 0.0)]
    fast["r"] = 0.5 * s
    fdelta = np.array([(30.0, 4.0, -18.0), (0.0, -44.0, 0.0), (-40.0, 0.0, 0.0), (-40.0, 0.0, 0.0)]) * s
    out["wide"] = _world(np.concatenate([w["comps"], fast]), np.concatenate([w["delta"], fdelta.astype(np.float32)]))
    for sc in out.values():
        sc["offset"], sc["size"] = o, s
    return out


ITERS = 4


def build_world(scene, new_world, new_mesh, new_obstacle):
    """the scene in a world of either implementation (the callables hide the two bindings' constructors): no gravity, unit masses"""
    w = new_world()
    if scene["mesh"] is not None:
        new_mesh(w, scene["mesh"])
    if scene["obstacle"] is not None:
        new_obstacle(w, scene["obstacle"])
    if len(scene["comps"]):
        w.add_bodies(scene["comps"], 1.0, 0.3, 0.6, (0.0, 0.0, 0.0))
    if scene["compound"] is not None:
        w.add_compound_bodies(scene["compound"]["comps"], 1.0, scene["compound"]["offsets"], 0.3, 0.6, (0.0, 0.0, 0.0))
    return w


def all_delta(scene):
    return scene["delta"] if scene["cdelta"] is None else np.concatenate([scene["delta"], scene["cdelta"]])


def constrain(w, scene, set_state):
    """build the constraint list of the planted cases: the whole front of a tick with dt = 1, no forces and v = the case's motion, so that
    integrate gives every body exactly that displacement.  (The collide phase alone is no way round: the tight boxes and the world-space
    parts it works on are made by begin_tick, in both implementations.)  integrate rebuilds every capsule from (x, q) - quat_from_arc -
    which nudges it by an ulp unless its axis is +y: the exact-parallel families keep their branches through the cases roll_axes turned
    that way, and tests/test_contact_corpus.py measures that they do."""
    set_state(w, v=all_delta(scene))
    return w.build_constraints(1.0)


def oracle_world(scene):
    from oracle import oracle as O

    def mesh(w, m):
        w.set_terrain(m["verts"], m["faces"], m["pos"])
    return build_world(scene, lambda: O.World(O.ORDER_CANONICAL), mesh, lambda w, ob: w.add_obstacle(ob))


def run_oracle_worlds(rungs=WORLD_RUNGS, names=None):
    """every world-form scene through the oracle's world (the load tests/test_contact_corpus.py measures); returns the constraint counts"""
    counts = {}
    for rung in rungs:
        for name, scene in world_scenes(rung).items():
            if names is not None and name not in names:
                continue
            w = oracle_world(scene)
            st = constrain(w, scene, lambda w_, **kw: w_.set_state(**kw))
            counts[(rung, name)] = (int(st.n_constraints), int(st.n_terrain_constraints))
    return counts


class LeafRecount:
    """The pair candidates of a world of single-component bodies counted from the leaf boxes alone, in f32 and in the reference's order
    (world.rs:233-260): body i's fat box is refitted when it no longer contains i's tight swept box, then every j < i whose fat box
    overlaps that tight box is a candidate.  The reference's own count comes out of its tree (bvh.rs:283-310), leaf AND ancestors - and an
    ancestor's box, (upper + lower) / 2 rounded to f32, can miss a child by an ulp of the coordinates: 1e5 from the origin a pair whose boxes
    touch exactly is lost there.  The HIP path's definition is this recount (include/mgf_hip.h, mgf_step_stats)."""

    def __init__(self, w):
        self.c, r = self._boxes(w)
        self.r = (r + np.float32(0.25)).astype(np.float32)

    @staticmethod
    def _boxes(w):
        import ctypes as C
        from oracle import oracle as O
        comps, delta = w.colliders()
        c, r = np.zeros((len(comps), 3), np.float32), np.zeros((len(comps), 3), np.float32)
        for i in range(len(comps)):
            b = O.Aabb()
            O.lib().mgfo_component_bounds(C.byref(O.Component(int(comps["tag"][i]), O.vec3(comps["p"][i]), O.vec3(comps["d"][i]), float(comps["r"][i]))),
                                          C.byref(O.vec3(delta[i])), C.byref(b))
            c[i], r[i] = b.c.tup(), b.r.tup()
        return c, r

    def count(self, w):
        """after a build_constraints of the oracle world w: the candidates of that tick"""
        tc, tr = self._boxes(w)
        total = 0
        for i in range(len(tc)):
            inside = np.all(np.abs(self.c[i] - (tc[i] + tr[i])) <= self.r[i]) and np.all(np.abs(self.c[i] - (tc[i] + -tr[i])) <= self.r[i])
            if not inside:
                self.c[i], self.r[i] = tc[i], tr[i] + np.float32(0.25)
            if i:
                total += int(np.all(np.abs(self.c[:i] - tc[i]) <= (self.r[:i] + tr[i]), axis=1).sum())
        return total


if __name__ == "__main__":   # python -m tests.contact_corpus: the number of cases per type, class and family
    cases = corpus()
    con, cnt = oracle_answers(cases)
    for t, v in classes(cases, con, cnt).items():
        print(f"{t:18s} {v}")
    t0, ty = con["t"][:, 0], case_type(cases)
    print(f"{'family':46s} {'cases':>7s} {'none':>7s} {'t = 0':>7s} {'t > 0':>7s} {'two':>7s}")
    for f, name in enumerate(FAMILIES):
        m = cases["family"] == f
        print(f"{name:46s} {m.sum():7d} {(m & (cnt == 0)).sum():7d} {(m & (cnt > 0) & (t0 == 0)).sum():7d} {(m & (cnt > 0) & (t0 > 0)).sum():7d} {(m & (cnt == 2)).sum():7d}")
