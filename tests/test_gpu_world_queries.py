"""Ray casts and box overlaps against a world's resident bodies, terrain and obstacles (mgf_world_raycast_many,
mgf_world_overlap_aabb_many).  The reference has no world query, so the definition is the build's (include/mgf_hip.h);
the expected answers are composed here from the oracle's own single-shape tests - oracle.intersection for a body's collider or
part and a terrain face, Compound.intersection for an obstacle - over the world's colliders, and compared bit for bit."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import scenes
from oracle import oracle as O

pytestmark = pytest.mark.gpu
INF = float("inf")
f32 = np.float32


def _direction_band():
    """(MGF_RAY_DMIN, MGF_RAY_DMAX) as include/mgf_hip.h states them"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgf_hip.h")) as f:
        text = f.read()
    return tuple(np.float32(re.search(r"#define\s+%s\s+([0-9.eE+-]+)f" % k, text).group(1)) for k in ("MGF_RAY_DMIN", "MGF_RAY_DMAX"))


RAY_DMIN, RAY_DMAX = _direction_band()


def ray_castable(d, band=None):
    """the rule of include/mgf_hip.h: a particle is cast only if the largest |component| of its direction lies in [DMIN, DMAX].
    band: another (DMIN, DMAX) - (0, inf) is the rule as it stood before the band: only d = 0 (or a NaN) hits nothing"""
    lo, hi = (RAY_DMIN, RAY_DMAX) if band is None else band
    m = np.abs(np.asarray(d, np.float32)).max()
    return bool(m > 0 and lo <= m <= hi)


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


# ---- the targets of a world, in the definition's order -----------------------------------------------------------------------
class Targets:
    def __init__(self, bodies, faces=None, obstacles=()):
        """bodies: a list, per caller index, of the body's components (COMPONENT rows in world coordinates); faces: (F, 3, 3)
        world-space triangles; obstacles: [(comps, disp, rot)]"""
        self.bodies = bodies
        self.faces = np.zeros((0, 3, 3), np.float32) if faces is None else faces
        self.obstacles = []
        for comps, disp, rot in obstacles:
            c = O.Compound([O.component(int(r["tag"]), r["p"], r["d"], float(r["r"])) for r in comps])
            c.set_pose(disp, rot)
            self.obstacles.append(c)
        flat = [(b, k, r) for b, parts in enumerate(bodies) for k, r in enumerate(parts)]
        self.owner = np.array([b for b, _, _ in flat], np.int64)
        self.part = np.array([k for _, k, _ in flat], np.int64)
        comps = np.array([r for _, _, r in flat], scenes.COMPONENT_DTYPE) if flat else np.zeros(0, scenes.COMPONENT_DTYPE)
        self.comps = comps
        # bounding spheres, padded: a cheap conservative filter in front of the oracle's tests
        d = comps["d"].astype(np.float64) * (comps["tag"] == 1)[:, None]
        self.bc = comps["p"].astype(np.float64) + 0.5 * d
        self.br = comps["r"].astype(np.float64) + 0.5 * np.linalg.norm(d, axis=1) + 1e-3
        fc = self.faces.astype(np.float64)
        self.fc = fc.mean(axis=1) if len(fc) else np.zeros((0, 3))
        self.fr = (np.linalg.norm(fc - self.fc[:, None, :], axis=2).max(axis=1) + 1e-3) if len(fc) else np.zeros(0)

    @staticmethod
    def _near(c, r, p, d, dt):
        p, d = np.asarray(p, np.float64), np.asarray(d, np.float64)
        dd = float(d @ d)
        if dd == 0.0:
            return np.linalg.norm(c - p, axis=1) <= r
        t = ((c - p) @ d) / dd
        t = np.clip(t, 0.0, dt if np.isfinite(dt) else np.inf)
        q = p + t[:, None] * d
        return np.linalg.norm(c - q, axis=1) <= r + 1e-6 * (1.0 + np.abs(p).max())

    def raycast(self, p, d, dt, ignore=-1, kinds=7, filtered=True, band=None):
        """the definition's answer (t, kind, index, part, point) or None.  filtered: only the targets whose bounding sphere the particle
        comes near are tried (_near) - right wherever the single tests are local; filtered=False puts every target of the world through
        the oracle's test (raycast_all), which is the definition itself"""
        if not filtered:
            return self.raycast_all(np.asarray(p, np.float32)[None], np.asarray(d, np.float32)[None], dt, ignore, kinds, band)[0]
        best = None  # (t, kind, index, part, point)
        if not ray_castable(d, band):
            return None  # a particle whose direction is outside the band hits nothing, d = 0 included (include/mgf_hip.h)

        def offer(res, kind, index, part):
            nonlocal best
            if res is None:
                return
            (ip, t) = res
            if not np.isfinite(t):
                return  # a hit whose t is not finite is not a candidate (include/mgf_hip.h)
            key = (t, kind, index, part)
            if best is None or key < best[:4]:
                best = (t, kind, index, part, ip)
        if kinds & 1 and len(self.comps):
            for e in np.nonzero(self._near(self.bc, self.br, p, d, dt))[0]:
                if self.owner[e] == ignore:
                    continue
                r = self.comps[e]
                sh = O.shape(O.SPHERE, r["p"], float(r["r"])) if r["tag"] == 0 else O.shape(O.CAPSULE, r["p"], r["d"], float(r["r"]))
                offer(O.intersection(p, d, dt, sh), 0, int(self.owner[e]), int(self.part[e]))
        if kinds & 2 and len(self.faces):
            for f in np.nonzero(self._near(self.fc, self.fr, p, d, dt))[0]:
                tri = self.faces[f]
                offer(O.intersection(p, d, dt, O.shape(O.TRIANGLE, tri[0], tri[1], tri[2])), 1, int(f), 0)
        if kinds & 4:
            for o, c in enumerate(self.obstacles):
                offer(c.intersection(p, d, dt), 2, o, None)
        return best

    def _all_shapes(self):
        """every component and every face as the oracle's shapes, components first"""
        if getattr(self, "_shapes", None) is None:
            sh = np.zeros(len(self.comps) + len(self.faces), O.SHAPE_DTYPE)
            nc = len(self.comps)
            cap = self.comps["tag"] == 1
            sh["kind"][:nc] = np.where(cap, O.CAPSULE, O.SPHERE)
            sh["v"][:nc, :3] = self.comps["p"]
            sh["v"][:nc, 3:6][cap] = self.comps["d"][cap]
            sh["v"][:nc, 6][cap] = self.comps["r"][cap]
            sh["v"][:nc, 3][~cap] = self.comps["r"][~cap]
            sh["kind"][nc:] = O.TRIANGLE
            sh["v"][nc:, :9] = self.faces.reshape(-1, 9)
            self._shapes = sh
        return self._shapes

    def raycast_all(self, p, d, dt, ignore=-1, kinds=7, band=None):
        """the unfiltered definition for n particles at once: every component, face and obstacle through the oracle's single test, then the
        least (t, kind, index, part).  Returns a list of (t, kind, index, part, point) or None"""
        p, d = np.ascontiguousarray(p, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n, nc = len(p), len(self.comps)
        dts = np.ascontiguousarray(np.broadcast_to(np.asarray(dt, np.float32), (n,)))
        ign = np.broadcast_to(np.asarray(ignore, np.int64), (n,))
        hit, ip, t = O.intersection_batch(p, d, dts, self._all_shapes(), every=True)
        ok = (hit == 1) & np.isfinite(t)
        if not kinds & 1:
            ok[:, :nc] = False
        if not kinds & 2:
            ok[:, nc:] = False
        if nc:
            ok[:, :nc] &= self.owner[None, :] != ign[:, None]
        # the columns stand in the definition's order (kind, index, part): the first least t of a row is its answer
        tt = np.where(ok, t, np.inf)
        col = np.argmin(tt, axis=1) if tt.shape[1] else np.zeros(n, np.int64)
        out = []
        for i in range(n):
            if not ray_castable(d[i], band):
                out.append(None)
                continue
            best = None
            if tt.shape[1] and ok[i, col[i]]:
                c = int(col[i])
                kind, index, part = (0, int(self.owner[c]), int(self.part[c])) if c < nc else (1, c - nc, 0)
                best = (float(t[i, c]), kind, index, part, tuple(float(x) for x in ip[i, c]))
            if kinds & 4:
                for o, c in enumerate(self.obstacles):
                    res = c.intersection(p[i], d[i], float(dts[i]))
                    if res is not None and np.isfinite(res[1]) and (best is None or (res[1], 2, o) < best[:3]):
                        best = (res[1], 2, o, None, res[0])
            out.append(best)
        return out

    def boxes(self):
        """BoundedBy<AABB> per body (bounds.rs:170-190), parts combined in order (box_combine, :113-130), in f32"""
        r = self.comps
        cap = r["tag"] == 1
        dv = np.where(cap[:, None], r["d"], np.float32(0)).astype(f32)
        m = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2], dtype=f32)
        rr = np.where(cap, r["r"] + m * f32(0.5), r["r"]).astype(f32)
        c = np.where(cap[:, None], r["p"] + dv * f32(0.5), r["p"]).astype(f32)
        h = np.repeat(rr[:, None], 3, axis=1)
        out = np.zeros((len(self.bodies), 6), np.float32)
        first = self.part == 0
        out[self.owner[first], :3], out[self.owner[first], 3:] = c[first], h[first]
        for k in range(1, int(self.part.max(initial=0)) + 1):
            sel = self.part == k
            b = self.owner[sel]
            bc, bh = out[b, :3], out[b, 3:]
            lo, hi = np.minimum(bc - bh, c[sel] - h[sel]), np.maximum(bc + bh, c[sel] + h[sel])
            out[b, 3:], out[b, :3] = (hi - lo) / f32(2), (hi + lo) / f32(2)
        return out


def world_targets(gw, scene=None, parts=None, obstacles=()):
    """the bodies as mgf_world_read_colliders returns them; `parts` replaces the colliders of bodies of several components
    (their world-space parts); the scene's terrain faces in world coordinates"""
    col = gw.colliders()
    comps = np.zeros(len(col), scenes.COMPONENT_DTYPE)
    for k in ("tag", "p", "d", "r"):
        comps[k] = col[k]
    bodies = [[comps[i]] for i in range(len(col))]
    if parts is not None:
        for i, ps in parts.items():
            bodies[i] = list(ps)
    faces = None
    if scene is not None and scene.get("terrain") is not None:
        t = scene["terrain"]
        v = np.asarray(t["verts"], np.float32).reshape(-1, 3) + np.asarray(t["pos"], np.float32)
        faces = v[np.asarray(t["faces"], np.int64).reshape(-1, 3)]
    return Targets(bodies, faces, obstacles)


def compare_rays(gw, T, p, d, dt, ignore=None, kinds=7):
    n = len(p)
    dts = np.broadcast_to(np.asarray(dt, np.float32), (n,))
    got = gw.raycast(p, d, dts, ignore=ignore, kinds=kinds)
    n_hits = 0
    for i in range(n):
        ign = -1 if ignore is None else int(np.broadcast_to(ignore, (n,))[i])
        want = T.raycast(p[i], d[i], float(dts[i]), ign, kinds)
        g = got[i]
        if want is None:
            assert g["kind"] == -1, (i, g, p[i], d[i])
            continue
        n_hits += 1
        t, kind, index, part, ip = want
        assert (g["kind"], g["index"]) == (kind, index), (i, g, want)
        if part is not None:
            assert g["part"] == part, (i, g, want)
        assert np.float32(g["t"]).view(np.uint32) == np.float32(t).view(np.uint32), (i, g["t"], t)
        assert np.array_equal(np.asarray(g["p"], np.float32).view(np.uint32), np.asarray(ip, np.float32).view(np.uint32)), (i, g, want)
    return got, n_hits


def compare_overlaps(gw, T, lo, hi):
    off, vals = gw.overlap_aabb(lo, hi)
    q = np.empty((len(lo), 6), np.float32)
    q[:, :3] = (np.asarray(hi, np.float32) + np.asarray(lo, np.float32)) / f32(2)
    q[:, 3:] = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / f32(2)
    bx = T.boxes()
    total = 0
    for i in range(len(lo)):
        ok = np.all(np.abs(bx[:, :3] - q[i, :3]) <= bx[:, 3:] + q[i, 3:], axis=1)  # collision.rs:22-29
        want = np.nonzero(ok)[0]
        assert np.array_equal(vals[off[i]:off[i + 1]], want), (i, vals[off[i]:off[i + 1]], want)
        total += len(want)
    return total


def rays_at(rng, centres, n, spread, up=8.0):
    """rays from above the bodies, pointing at (near) them; segments of several lengths"""
    tgt = centres[rng.integers(0, len(centres), n)] + rng.normal(0, spread, (n, 3))
    p = tgt + rng.normal(0, 1.0, (n, 3)) + np.array([0.0, up, 0.0])
    d = (tgt - p)
    return p.astype(np.float32), d.astype(np.float32)


def some_boxes(rng, centres, n, width):
    c = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.5, (n, 3))
    h = rng.uniform(0.5, 2.0, (n, 1)) * width * 0.5 * np.ones((1, 3))
    return (c - h).astype(np.float32), (c + h).astype(np.float32)


# ---- config 1 ----------------------------------------------------------------------------------------------------------------
def test_balls_demo_after_a_few_ticks(ctx):
    sc = scenes.balls_demo(8)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 30)
    T = world_targets(gw, sc)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(1)
    p, d = rays_at(rng, cen, 96, 0.4)
    _, hits = compare_rays(gw, T, p, d, INF)
    assert hits > 48
    # segments: ending short of, exactly at and beyond the first hit
    got = gw.raycast(p, d, INF, kinds=1)
    hit = (got["kind"] == 0) & (got["t"] > 0)
    ts = got["t"][hit].astype(np.float32)
    for scale in (np.float32(0.5), np.float32(1.0), np.float32(1.5)):
        dseg = (d[hit] * (ts * scale)[:, None]).astype(np.float32)
        compare_rays(gw, T, p[hit], dseg, 1.0)
    # grazing: horizontal rays at the height of the top of a ball, the terrain's walls behind them
    top = cen[rng.integers(0, len(cen), 48)] + np.array([0.0, 0.5, 0.0], np.float32)
    pg = (top + np.array([-15.0, 0.0, 0.0], np.float32)).astype(np.float32)
    dg = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (48, 1))
    compare_rays(gw, T, pg, dg, INF)
    # straight down onto the floor between the balls, terrain only and all kinds
    pf = np.stack([rng.uniform(-9, 9, 64), np.full(64, 30.0), rng.uniform(-9, 9, 64)], axis=1).astype(np.float32)
    df = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (64, 1))
    for kinds in (1, 2, 3, 7):
        compare_rays(gw, T, pf, df, INF, kinds=kinds)
    lo, hi = some_boxes(rng, cen, 64, 1.0)
    assert compare_overlaps(gw, T, lo, hi) > 0


# ---- capsules over a heightfield ------------------------------------------------------------------------------------------------
def test_capsules_over_a_heightfield(ctx):
    sc = scenes.capsule_field(8, 2, 8, quads=12)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 15)
    T = world_targets(gw, sc)
    shp = gw.colliders()
    cen = shp["p"] + 0.5 * shp["d"]
    rng = np.random.default_rng(2)
    p, d = rays_at(rng, cen, 96, 0.6)
    compare_rays(gw, T, p, d, INF)
    # rays along the terrain, a little above it and from outside the field, both directions
    v = T.faces.reshape(-1, 3)
    ext = v.min(axis=0), v.max(axis=0)
    y = rng.uniform(ext[0][1], ext[1][1] + 0.5, 64)
    z = rng.uniform(ext[0][2], ext[1][2], 64)
    pa = np.stack([np.full(64, ext[0][0] - 5.0), y, z], axis=1).astype(np.float32)
    da = np.stack([np.ones(64), rng.uniform(-0.05, 0.05, 64), rng.uniform(-0.05, 0.05, 64)], axis=1).astype(np.float32)
    compare_rays(gw, T, pa, da, INF)
    compare_rays(gw, T, pa, da, INF, kinds=2)
    lo, hi = some_boxes(rng, cen, 48, 3.0)
    compare_overlaps(gw, T, lo, hi)


# ---- bodies of several components --------------------------------------------------------------------------------------------
def _compound_parts(sc):
    cb = sc["compound"]
    n0 = len(sc["comps"])
    off = cb["offsets"]
    return {n0 + b: cb["comps"][off[b]:off[b + 1]] for b in range(len(off) - 1)}


@pytest.mark.parametrize("name", ["dumbbells", "caterpillars"])
def test_bodies_of_several_parts(ctx, name):
    """world-space parts as added (a world that has not been stepped sees them there), two-part bodies and bodies of the pool"""
    sc = scenes.dumbbell_field(5, 2, 5, n_plain=12) if name == "dumbbells" else scenes.caterpillar_field(3, 2, 3, n_plain=6, small_every=4)
    gw = mgf_amd.World.from_scene(ctx, sc)
    parts = _compound_parts(sc)
    T = world_targets(gw, sc, parts=parts)
    allp = np.concatenate([np.asarray(v["p"], np.float32) for v in parts.values()])
    rng = np.random.default_rng(3)
    p, d = rays_at(rng, allp, 128, 0.3)
    got, hits = compare_rays(gw, T, p, d, INF)
    hit_parts = got["part"][(got["kind"] == 0) & np.isin(got["index"], list(parts))]
    assert hits > 32 and hit_parts.max() > 0  # parts other than the first answer
    lo, hi = some_boxes(rng, allp, 48, 2.0)
    compare_overlaps(gw, T, lo, hi)


# ---- obstacles, the tie rule, kinds, ignore ----------------------------------------------------------------------------------
def _tie_world(ctx):
    comps = np.zeros(5, scenes.COMPONENT_DTYPE)
    comps["tag"] = [0, 0, 1, 0, 0]
    comps["p"] = [(0, 5, 0), (0, 5, 0), (4, 3, -1), (-4, 2, 0), (8, 5, 0)]
    comps["d"] = [(0, 0, 0), (0, 0, 0), (0, 0, 2), (0, 0, 0), (0, 0, 0)]
    comps["r"] = [0.5, 0.5, 0.4, 0.7, 0.5]
    gw = mgf_amd.World(ctx)
    gw.add_bodies(comps, np.ones(5, np.float32), np.zeros(5, np.float32), np.full(5, 0.5, np.float32), np.zeros((5, 3), np.float32))
    # obstacle 0: a sphere exactly where bodies 0 and 1 are, and another one elsewhere; obstacle 1: a sphere that its pose puts where body 4 is
    o0 = np.zeros(2, scenes.COMPONENT_DTYPE)
    o0["tag"] = 0
    o0["p"] = [(0, 5, 0), (0, 0, 6)]
    o0["r"] = [0.5, 1.0]
    o1 = np.zeros(1, scenes.COMPONENT_DTYPE)
    o1["tag"] = 0
    o1["p"] = [(8, 5.5, 0)]
    o1["r"] = [0.5]
    obs = [(o0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)), (o1, (0.0, -0.5, 0.0), (1.0, 0.0, 0.0, 0.0))]
    for c, disp, rot in obs:
        k = mgf_amd.Compound(ctx, c)
        k.set_pose(disp, rot)
        gw.add_obstacle(k)
    return gw, obs


def test_obstacles_ties_kinds_and_ignore(ctx):
    gw, obs = _tie_world(ctx)
    T = world_targets(gw, obstacles=obs)
    p = np.array([(0, 10, 0), (0, 10, 0.2), (8, 10, 0), (0, 2, 6), (4, 10, 0), (-4, 10, 0.3), (0, 5, 0), (0, 5, 0)], np.float32)
    d = np.tile(np.array([0, -1, 0], np.float32), (len(p), 1))
    d[6] = (1, 0, 0)
    d[7] = (0, 1, 0)
    for kinds in range(1, 8):
        got, _ = compare_rays(gw, T, p, d, INF, kinds=kinds)
    got = gw.raycast(p, d, INF)
    # the same t on two bodies and an obstacle: the body with the smaller caller index
    assert (got[0]["kind"], got[0]["index"]) == (0, 0) and (got[2]["kind"], got[2]["index"]) == (0, 4)
    got = gw.raycast(p[:1], d[:1], INF, kinds=4)
    assert (got[0]["kind"], got[0]["index"], got[0]["part"]) == (2, 0, 0)
    got = gw.raycast(p[3:4], d[3:4], INF, kinds=4)
    assert (got[0]["kind"], got[0]["index"], got[0]["part"]) == (2, 0, 1)
    # cast from inside a body: itself at t = 0, or - ignored - what lies behind it
    ign = np.array([-1, 0, 4, -1, 2, 3, 0, 1], np.int32)
    compare_rays(gw, T, p, d, INF, ignore=ign)
    got = gw.raycast(p[6:], d[6:], INF, ignore=[0, 0])
    assert got[0]["kind"] == 0 and got[0]["index"] == 1 and got[0]["t"] == 0.0
    got = gw.raycast(p[6:7], d[6:7], INF, ignore=[-1])
    assert got[0]["index"] == 0 and got[0]["t"] == 0.0
    # no direction: no hit, even from inside a body
    assert gw.raycast(p[6:7], np.zeros((1, 3), np.float32), 1.0)[0]["kind"] == -1
    # segments that end exactly on the surface (t = 1) and just short of it
    seg = np.array([[0, 5.5, 0], [0, 5.5001, 0]], np.float32) - p[:1]
    compare_rays(gw, T, np.repeat(p[:1], 2, axis=0), seg, 1.0)
    compare_overlaps(gw, T, np.array([[-1, 4, -1], [3, 0, -3], [50, 50, 50]], np.float32), np.array([[1, 6, 1], [9, 9, 3], [51, 51, 51]], np.float32))


def test_a_world_with_obstacles_after_ticks(ctx):
    sc = scenes.capsule_field_dense(6, 3, 6, y0=2.5, sphere_fraction=0.4)
    gw = mgf_amd.World.from_scene(ctx, sc)
    import tests.test_gpu_obstacles as tob
    obs = tob._obstacles()
    for comps, disp, rot in obs:
        k = mgf_amd.Compound(ctx, comps)
        k.set_pose(disp, rot)
        gw.add_obstacle(k)
    gw.step_many(float(sc["dt"]), sc["iters"], 10)
    T = world_targets(gw, sc, obstacles=obs)
    shp = gw.colliders()
    rng = np.random.default_rng(4)
    aim = np.concatenate([shp["p"], np.array([[0.4, 0.6, -0.3], [-1.0, 0.5, 1.5], [1.5, 0.5, 1.5]], np.float32)])
    p, d = rays_at(rng, aim, 128, 1.0)
    for kinds in (7, 5, 4, 6):
        compare_rays(gw, T, p, d, INF, kinds=kinds)
    compare_rays(gw, T, p, d * np.float32(0.7), 1.0)


# ---- a re-sorted store, a runaway body ---------------------------------------------------------------------------------------
def test_resorted_store_reports_caller_indices(ctx):
    sc = scenes.sphere_pile(12, 6, 12)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.set_option("resort_every", 2)
    gw.step_many(float(sc["dt"]), sc["iters"], 7)
    T = world_targets(gw, sc)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(5)
    p, d = rays_at(rng, cen, 128, 0.4, up=12.0)
    _, hits = compare_rays(gw, T, p, d, INF)
    assert hits > 64
    lo, hi = some_boxes(rng, cen, 64, 2.0)
    compare_overlaps(gw, T, lo, hi)


def test_a_runaway_body_goes_to_the_large_list(ctx):
    sc = scenes.sphere_pile(8, 4, 8)
    comps = np.concatenate([sc["comps"], np.zeros(1, scenes.COMPONENT_DTYPE)])
    comps[-1]["tag"] = 1
    comps[-1]["p"] = (-150.0, 20.0, 0.0)
    comps[-1]["d"] = (300.0, 0.0, 0.0)
    comps[-1]["r"] = 0.5
    n = len(comps)
    gw = mgf_amd.World(ctx)
    gw.add_bodies(comps, np.ones(n, np.float32), np.zeros(n, np.float32), np.full(n, 0.5, np.float32), np.zeros((n, 3), np.float32))
    T = world_targets(gw)
    cen = comps["p"][:-1]
    rng = np.random.default_rng(6)
    p, d = rays_at(rng, cen, 96, 0.4, up=30.0)
    got, _ = compare_rays(gw, T, p, d, INF)
    assert np.any(got["index"] == n - 1)
    assert gw.counter("query_large_bodies") >= 1
    lo, hi = some_boxes(rng, cen, 32, 2.0)
    compare_overlaps(gw, T, np.concatenate([lo, [[-1, 19, -1]]]).astype(np.float32), np.concatenate([hi, [[1, 21, 1]]]).astype(np.float32))


def test_overlap_capacity_contract(ctx):
    sc = scenes.sphere_pile(6, 4, 6)
    gw = mgf_amd.World.from_scene(ctx, sc)
    cen = gw.colliders()["p"]
    lo = (cen[:8] - 1.0).astype(np.float32)
    hi = (cen[:8] + 1.0).astype(np.float32)
    boxes = np.concatenate([(hi + lo) / 2, (hi - lo) / 2], axis=1).astype(np.float32)
    off, vals = gw.overlap_boxes(boxes)
    assert len(vals) == off[-1] > 8
    with pytest.raises(mgf_amd.MgfError) as e:
        gw.overlap_boxes(boxes, cap=len(vals) - 1)
    assert e.value.status == mgf_amd._capi.ERR_CAPACITY
    import ctypes as C
    o2 = np.zeros(len(boxes) + 1, np.uint64)
    tot = C.c_int64()
    v2 = np.zeros(3, np.uint32)
    st = mgf_amd.load_library().mgf_world_overlap_aabb_many(gw._h, boxes.ctypes.data, len(boxes), o2.ctypes.data, v2.ctypes.data, 3, C.byref(tot))
    assert st == mgf_amd._capi.ERR_CAPACITY and tot.value == len(vals) and np.array_equal(o2.astype(np.int64), off)


# ---- a tile set: ghosts are not reported ---------------------------------------------------------------------------------------
def test_ghosts_are_never_reported(ctx):
    import torch
    sc = scenes.sphere_pile(8, 4, 8)
    n = len(sc["comps"])
    dt = float(sc["dt"])
    gw = mgf_amd.World.from_scene(ctx, sc)
    other = mgf_amd.World.from_scene(ctx, sc)
    # every body of `other` as a ghost of gw, at the same place: a query that saw ghosts would find twice the bodies
    other.begin_tick(dt)
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    recs = torch.zeros((n, 72), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the fill runs on torch's stream, the library writes on its own)
    other.export_bodies(ids.data_ptr(), n, recs.data_ptr())
    gw.begin_tick(dt)
    gw.import_ghosts(recs.data_ptr(), n)
    assert gw.ghost_len() == n and len(gw) == n
    T = world_targets(gw, sc)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(7)
    p, d = rays_at(rng, cen, 64, 0.4)
    got, hits = compare_rays(gw, T, p, d, INF)
    assert hits > 0 and got["index"].max() < n
    lo, hi = some_boxes(rng, cen, 32, 2.0)
    off, vals = gw.overlap_aabb(lo, hi)
    assert vals.max() < n
    compare_overlaps(gw, T, lo, hi)
    torch.cuda.synchronize()


# ---- queries do not disturb the tick -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [False, True])
def test_queries_leave_the_tick_bit_identical(ctx, many):
    sc = scenes.sphere_pile(10, 6, 10)
    a, b = mgf_amd.World.from_scene(ctx, sc), mgf_amd.World.from_scene(ctx, sc)
    for w in (a, b):
        w.set_option("resort_every", 2)
    dt, iters = float(sc["dt"]), sc["iters"]
    rng = np.random.default_rng(8)
    for k in range(5 if many else 10):
        if many:
            a.step_many(dt, iters, 2)
            b.step_many(dt, iters, 2)
        else:
            a.step(dt, iters)
            b.step(dt, iters)
        cen = a.colliders()["p"]
        p, d = rays_at(rng, cen, 64, 0.5)
        a.raycast(p, d)
        lo, hi = some_boxes(rng, cen, 16, 2.0)
        a.overlap_aabb(lo, hi)
    sa, sb = a.state(), b.state()
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]).view(np.uint32), np.asarray(sb[key]).view(np.uint32)), key
    ca, cb = a.constraints(), b.constraints()
    assert len(ca) == len(cb) > 0 and ca.tobytes() == cb.tobytes()


# ---- full size once ----------------------------------------------------------------------------------------------------------
def test_config_2_full_size(ctx):
    sc = scenes.config(1)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 3)
    T = world_targets(gw, sc)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(9)
    p, d = rays_at(rng, cen, 4096, 1.0, up=4.0)
    dt = np.where(rng.random(4096) < 0.5, np.float32(INF), np.float32(1.0)).astype(np.float32)
    got = gw.raycast(p, d, dt)
    for i in range(0, 4096):
        want = T.raycast(p[i], d[i], float(dt[i]))
        g = got[i]
        if want is None:
            assert g["kind"] == -1, i
        else:
            assert (g["kind"], g["index"], np.float32(g["t"]).view(np.uint32)) == (want[1], want[2], np.float32(want[0]).view(np.uint32)), (i, g, want)
            assert np.array_equal(np.asarray(g["p"], np.float32).view(np.uint32), np.asarray(want[4], np.float32).view(np.uint32)), i
    lo, hi = some_boxes(rng, cen, 1024, 2.0)
    assert compare_overlaps(gw, T, lo, hi) > 1024
