"""Swept spheres and capsules against a world's resident bodies, terrain and obstacles (mgf_world_sweep_many).  The reference has no
world query, so the definition is the build's (include/mgf_hip.h); the expected answers are composed here from the oracle's own
continuous tests - oracle.contacts(target, None, cast, delta) for a body's collider or part and a terrain face, Compound.contacts for
an obstacle - over the world's colliders, and compared bit for bit: kind, index, part and the ten floats of the contact."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import mgf_amd
from mgf_amd import scenes
from oracle import oracle as O
from tests.test_gpu_world_queries import _compound_parts, _tie_world, world_targets

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _shape(tag, p, d, r):
    return O.shape(O.SPHERE, p, float(r)) if int(tag) == 0 else O.shape(O.CAPSULE, p, d, float(r))


class Sweeper:
    """The definition's answer for one cast, composed from the single tests.  A candidate is tested only if its bounding sphere comes
    within reach of the cast's along the path (a cheap conservative filter), and in the order of the earliest t that filter allows, up
    to the best t found so far."""

    def __init__(self, T, obstacles=()):
        self.T = T
        self.tree = cKDTree(T.bc) if len(T.bc) else None
        self.brmax = float(T.br.max()) if len(T.br) else 0.0
        self.shapes = {}
        # each obstacle's components one by one, at its pose: the component a contact of Compound.contacts came from
        self.singles = []
        for comps, disp, rot in obstacles:
            one = []
            for r in comps:
                c = O.Compound([O.component(int(r["tag"]), r["p"], r["d"], float(r["r"]))])
                c.set_pose(disp, rot)
                one.append(c)
            self.singles.append(one)
        self.n_nonfinite = 0  # contacts with a t that is not finite, which the definition leaves out

    def _body_shape(self, e):
        s = self.shapes.get(e)
        if s is None:
            r = self.T.comps[e]
            s = self.shapes[e] = _shape(r["tag"], r["p"], r["d"], r["r"])
        return s

    @staticmethod
    def _t_lo(c, R, cc, v):
        """the earliest t in [0, 1] at which spheres (c, R) may meet the point cc + t v, minus a little; inf: never"""
        w = c - cc
        vv = float(v @ v)
        ww = np.einsum("ij,ij->i", w, w)
        inside = ww <= R * R
        if vv == 0.0:
            return np.where(inside, 0.0, np.inf)
        wv = w @ v
        disc = wv * wv - vv * (ww - R * R)
        t = (wv - np.sqrt(np.maximum(disc, 0.0))) / vv
        t = np.where(disc < 0, np.inf, t)
        t = np.where(inside, 0.0, t)
        t = np.where(t > 1.0 + 1e-6, np.inf, t)
        return np.where(np.isfinite(R) | inside, np.maximum(t - 1e-6, 0.0), 0.0)

    def answer(self, cast, ignore=-1, kinds=7, filtered=True):
        """filtered=False: every body's component and every face is put through the oracle's test, whatever its bounding sphere says -
        the definition itself; the filter is right wherever the single tests are local"""
        T = self.T
        tag, p, d, r, v = int(cast["tag"]), cast["p"].astype(np.float64), cast["d"].astype(np.float64), float(cast["r"]), cast["delta"].astype(np.float64)
        sh = _shape(tag, cast["p"], cast["d"], r)
        dv = d if tag == 1 else np.zeros(3)
        cc = p + 0.5 * dv
        with np.errstate(over="ignore", invalid="ignore"):
            rc = r + 0.5 * np.linalg.norm(dv) + 1e-3 + 1e-5 * (np.abs(cc).max() + np.abs(v).max())
        vec = cast["delta"]
        best = None  # (t, kind, index, part, order, contact)

        def offer(res, kind, index, part_of):
            nonlocal best
            for j, c in enumerate(res):
                t = c["t"]
                if not np.isfinite(t):
                    self.n_nonfinite += 1
                    continue
                key = (t, kind, index, part_of(c), j)
                if best is None or key < best[:5]:
                    best = key + (c,)

        cands = []  # (t_lo, kind, index)
        if kinds & 1 and len(T.comps):
            if filtered and np.isfinite(rc) and np.all(np.isfinite(cc)):
                mid = cc + 0.5 * v
                idx = np.array(self.tree.query_ball_point(mid, 0.5 * np.linalg.norm(v) + rc + self.brmax), np.int64)
            else:
                idx = np.arange(len(T.comps))
            if len(idx):
                tl = self._t_lo(T.bc[idx], T.br[idx] + rc, cc, v) if filtered else np.zeros(len(idx))
                cands += [(t, 0, int(e)) for t, e in zip(tl, idx) if np.isfinite(t) and T.owner[e] != ignore]
        if kinds & 2 and len(T.faces):
            reach = 0.0 if tag == 0 else max(1.0, float(np.linalg.norm(d)))  # a capsule's face test reaches further (include/mgf_hip.h)
            tl = self._t_lo(T.fc, T.fr + rc + reach, cc, v)
            d32 = cast["delta"].astype(f32)
            if tag == 1 and (d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2] == 0:
                tl = np.zeros(len(T.faces))  # a capsule that does not move may meet any face at t = 0 (include/mgf_hip.h)
            if not filtered:
                tl = np.zeros(len(T.faces))
            cands += [(t, 1, int(f)) for f, t in enumerate(tl) if np.isfinite(t)]
        if kinds & 4:
            for o, comp in enumerate(T.obstacles):
                res = comp.contacts(sh, vec)

                def part_of(c, o=o):
                    ks = [k for k, one in enumerate(self.singles[o]) if any(_same(c, x) for x in one.contacts(sh, vec))]
                    assert ks, ("an obstacle's contact matches none of its components", o, c)
                    return ks[0]
                offer(res, 2, o, part_of)
        cands.sort()
        for t_lo, kind, i in cands:
            if filtered and best is not None and t_lo > best[0] + 1e-6:
                break
            if kind == 0:
                offer(O.contacts(self._body_shape(i), None, sh, vec), 0, int(T.owner[i]), lambda c, i=i: int(T.part[i]))
            else:
                tri = T.faces[i]
                offer(O.contacts(O.shape(O.TRIANGLE, tri[0], tri[1], tri[2]), None, sh, vec), 1, i, lambda c: 0)
        return best


def answer_all(T, casts, ignore=-1, kinds=3, obstacles=()):
    """The unfiltered definition for n casts at once: every component and every face of T through the oracle's continuous test
    (contacts_batch: the target at rest, the cast moving) and, with kinds & 4, every obstacle of `obstacles` [(comps, disp, rot)] through
    Compound.contacts (the component a contact came from found as Sweeper finds it), then the least (t, kind, index, part, order) among
    the contacts whose t is finite.  A list of what Sweeper.answer returns."""
    if kinds & 4 and len(obstacles):
        S = Sweeper(T, obstacles)
        rest = answer_all(T, casts, ignore, kinds & 3) if kinds & 3 else [None] * len(casts)
        out = []
        for i, best in enumerate(rest):
            sh = _shape(casts["tag"][i], casts["p"][i], casts["d"][i], casts["r"][i])
            for o, comp in enumerate(T.obstacles):
                for j, c in enumerate(comp.contacts(sh, casts["delta"][i])):
                    if not np.isfinite(c["t"]):
                        continue
                    ks = [k for k, one in enumerate(S.singles[o]) if any(_same(c, x) for x in one.contacts(sh, casts["delta"][i]))]
                    assert ks, ("an obstacle's contact matches none of its components", o, c)
                    key = (float(c["t"]) + 0.0, 2, o, ks[0], j)
                    if best is None or key < (best[0] + 0.0,) + tuple(best[1:5]):
                        best = key + (c,)
            out.append(best)
        return out
    kinds &= 3
    if not kinds:
        return [None] * len(casts)
    sh = T._all_shapes()
    n, m, nc = len(casts), len(sh), len(T.comps)
    B = np.zeros(n, O.SHAPE_DTYPE)
    cap = casts["tag"] == 1
    B["kind"] = np.where(cap, O.CAPSULE, O.SPHERE)
    B["v"][:, :3] = casts["p"]
    B["v"][:, 3:6][cap] = casts["d"][cap]
    B["v"][:, 6][cap] = casts["r"][cap]
    B["v"][:, 3][~cap] = casts["r"][~cap]
    if m == 0:
        return [None] * n
    con, cnt = O.contacts_batch(np.tile(sh, n), np.zeros((n * m, 3), f32), np.repeat(B, m), np.repeat(casts["delta"], m, axis=0), np.full(n * m, 2, np.uint8), slots=2)
    con, cnt = con.reshape(n, m, 2), cnt.reshape(n, m)
    ok = (np.arange(2)[None, None, :] < cnt[:, :, None]) & np.isfinite(con["t"])
    ign = np.broadcast_to(np.asarray(ignore, np.int64), (n,))
    if nc:
        ok[:, :nc] &= (T.owner[None, :] != ign[:, None])[:, :, None]
    if not kinds & 1:
        ok[:, :nc] = False
    if not kinds & 2:
        ok[:, nc:] = False
    tt = np.where(ok, con["t"], np.inf).reshape(n, 2 * m)   # columns in the definition's order: (kind, index, part), order emitted within
    col = np.argmin(tt, axis=1)
    out = []
    for i in range(n):
        c, j = divmod(int(col[i]), 2)
        if not ok[i, c, j]:
            out.append(None)
            continue
        kind, index, part = (0, int(T.owner[c]), int(T.part[c])) if c < nc else (1, c - nc, 0)
        k = con[i, c, j]
        out.append((float(k["t"]), kind, index, part, j, dict(a=tuple(k["a"]), b=tuple(k["b"]), n=tuple(k["n"]), t=k["t"])))
    return out


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k], f32).view(np.uint32), np.asarray(b[k], f32).view(np.uint32)) for k in ("a", "b", "n", "t"))


def compare_sweeps(gw, S, casts, ignore=None, kinds=7):
    got = gw.sweep(casts, ignore=ignore, kinds=kinds)
    n = len(casts)
    ign = np.full(n, -1) if ignore is None else np.broadcast_to(np.asarray(ignore), (n,))
    n_hits, wants = 0, []
    for i in range(n):
        want = S.answer(casts[i], int(ign[i]), kinds)
        wants.append(want)
        g = got[i]
        if want is None:
            assert g["kind"] == -1 and g["index"] == 0 and g["part"] == 0, (i, g, casts[i])
            assert np.all(np.asarray([g["a"], g["b"], g["n"]]) == 0) and g["t"] == 0.0, (i, g)
            continue
        n_hits += 1
        t, kind, index, part, _, c = want
        assert (g["kind"], g["index"], g["part"]) == (kind, index, part), (i, g, want, casts[i])
        assert _same(c, {k: g[k] for k in ("a", "b", "n", "t")}), (i, g, want, casts[i])
    return got, n_hits, wants


def casts_at(rng, centres, n, spread, length, r=(0.2, 0.6), capsule_len=(0.3, 1.5)):
    """half spheres, half capsules, from around the centres aimed at (near) others; sweep lengths drawn from `length` (a pair: uniform)"""
    c = np.zeros(n, mgf_amd.MOVING_DTYPE)
    src = centres[rng.integers(0, len(centres), n)] + rng.normal(0, spread, (n, 3)) + np.array([0.0, 1.5, 0.0])
    tgt = centres[rng.integers(0, len(centres), n)] + rng.normal(0, spread, (n, 3))
    dirn = tgt - src
    dirn /= np.maximum(np.linalg.norm(dirn, axis=1, keepdims=True), 1e-9)
    ln = rng.uniform(length[0], length[1], n)
    c["tag"] = np.arange(n) % 2
    c["r"] = rng.uniform(r[0], r[1], n)
    ax = rng.normal(0, 1, (n, 3))
    ax *= (rng.uniform(capsule_len[0], capsule_len[1], n) / np.linalg.norm(ax, axis=1))[:, None]
    c["d"] = np.where((c["tag"] == 1)[:, None], ax, 0.0)
    c["p"] = src - 0.5 * c["d"]
    c["delta"] = dirn * ln[:, None]
    return c


def _cast(tag, p, d, r, delta):
    c = np.zeros(1, mgf_amd.MOVING_DTYPE)
    c["tag"], c["p"], c["d"], c["r"], c["delta"] = tag, p, d, r, delta
    return c


# ---- config 1: short, long, zero-length, from inside -------------------------------------------------------------------------
def test_balls_demo_after_a_few_ticks(ctx):
    sc = scenes.balls_demo(8)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 30)
    T = world_targets(gw, sc)
    S = Sweeper(T)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(11)
    short = casts_at(rng, cen, 96, 0.4, (0.05, 0.9))
    long = casts_at(rng, cen, 96, 0.4, (4.0, 20.0))
    zero = casts_at(rng, cen, 64, 0.4, (0.0, 0.0))
    inside = casts_at(rng, cen, 64, 0.0, (0.0, 3.0))
    inside["p"] = cen[rng.integers(0, len(cen), 64)] - 0.5 * inside["d"] + rng.normal(0, 0.1, (64, 3))
    inside["delta"][:32] = 0.0
    casts = np.concatenate([short, long, zero, inside])
    got, hits, _ = compare_sweeps(gw, S, casts)
    assert hits > 150
    k = got["kind"]
    assert np.any(k[:96] >= 0) and np.any(k[96:192] >= 0)
    # zero-length casts of both kinds that start overlapping a body answer at t = 0
    z, zt = got[256:288], inside["tag"][:32]
    assert np.any((z["kind"] == 0) & (z["t"] == 0) & (zt == 0)) and np.any((z["kind"] == 0) & (z["t"] == 0) & (zt == 1))
    # sphere on sphere with equal centres: nothing (collision.rs:1097-1100); a capsule there answers
    b0 = gw.colliders()[0]
    same = np.concatenate([_cast(0, b0["p"], (0, 0, 0), 0.3, (0, 0, 0)), _cast(1, b0["p"] + (-0.2, 0.1, 0), (0.4, 0, 0), 0.3, (0, 0, 0))])
    got, _, _ = compare_sweeps(gw, S, same, kinds=1)
    assert got[0]["kind"] == -1 or got[0]["index"] != 0
    assert got[1]["kind"] == 0 and got[1]["t"] == 0.0


# ---- capsules over a heightfield: the two-contact case and its order ------------------------------------------------------------
def test_capsules_over_a_heightfield(ctx):
    sc = scenes.capsule_field(8, 2, 8, quads=12)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 15)
    T = world_targets(gw, sc)
    S = Sweeper(T)
    shp = gw.colliders()
    cen = shp["p"] + 0.5 * shp["d"]
    rng = np.random.default_rng(12)
    casts = casts_at(rng, cen, 128, 0.6, (0.0, 6.0))
    compare_sweeps(gw, S, casts)
    # capsules lying parallel to a face, swept straight down onto it, and along it at its height; terrain only and all kinds
    tri = T.faces
    n = min(len(tri), 48)
    pick = rng.choice(len(tri), n, replace=False)
    a, b, c = tri[pick, 0].astype(np.float64), tri[pick, 1].astype(np.float64), tri[pick, 2].astype(np.float64)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.sign(nrm[:, 1:2])
    ctr = (a + b + c) / 3.0
    edge = (b - a) * 0.3
    par = np.zeros(3 * n, mgf_amd.MOVING_DTYPE)
    par["tag"] = 1
    par["r"] = 0.25
    par["d"][:n] = edge                        # parallel to the face, above its centre, swept down along the normal
    par["p"][:n] = ctr - 0.5 * edge + nrm * 1.0
    par["delta"][:n] = -nrm * 2.0
    par["d"][n:2 * n] = b - a                  # along an edge, lifted by the radius plus a little, swept down
    par["p"][n:2 * n] = a + nrm * 0.5
    par["delta"][n:2 * n] = -nrm * 1.0
    par["d"][2 * n:] = edge                    # lying on the face already: zero-length
    par["p"][2 * n:] = ctr - 0.5 * edge + nrm * 0.2
    got, hits, wants = compare_sweeps(gw, S, par, kinds=2)
    compare_sweeps(gw, S, par)
    assert hits > n
    # the two-contact case occurs, and where both contacts share t the first emitted one is the answer
    two = 0
    for i, w in enumerate(wants):
        if w is None:
            continue
        res = O.contacts(O.shape(O.TRIANGLE, *T.faces[w[2]]), None, _shape(1, par[i]["p"], par[i]["d"], par[i]["r"]), par[i]["delta"])
        if len(res) == 2 and res[0]["t"] == res[1]["t"]:
            two += 1
            assert _same(res[0], {k: got[i][k] for k in ("a", "b", "n", "t")})
    assert two > 0
    # a capsule whose length overflows f32: the face test emits t = NaN (here for every face the cast is near), and NaN is never
    # the answer.  (Its finite contacts are not compared: at these magnitudes the device's face test is not held to the oracle.)
    huge = np.concatenate([_cast(1, ctr[k] + nrm[k] * 0.6, (-3e38, -0.16, -0.48), 0.3, (1.2, -0.8, -0.6)) for k in range(8)])
    sh = [_shape(1, c["p"], c["d"], c["r"]) for c in huge]
    nan_faces = [[f for f in range(len(tri)) if any(np.isnan(x["t"]) for x in O.contacts(O.shape(O.TRIANGLE, *tri[f]), None, sh[k], huge[k]["delta"]))]
                 for k in range(len(huge))]
    assert all(len(f) > 0 for f in nan_faces)
    got = gw.sweep(huge, kinds=2)
    assert np.all(np.isfinite(got["t"]))


# ---- bodies of several components ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dumbbells", "caterpillars"])
def test_bodies_of_several_parts(ctx, name):
    sc = scenes.dumbbell_field(5, 2, 5, n_plain=12) if name == "dumbbells" else scenes.caterpillar_field(3, 2, 3, n_plain=6, small_every=4)
    gw = mgf_amd.World.from_scene(ctx, sc)
    parts = _compound_parts(sc)
    T = world_targets(gw, sc, parts=parts)
    S = Sweeper(T)
    allp = np.concatenate([np.asarray(v["p"], np.float32) for v in parts.values()])
    rng = np.random.default_rng(13)
    casts = casts_at(rng, allp, 128, 0.3, (0.0, 5.0))
    got, hits, _ = compare_sweeps(gw, S, casts)
    hit_parts = got["part"][(got["kind"] == 0) & np.isin(got["index"], list(parts))]
    assert hits > 32 and hit_parts.max() > 0


# ---- obstacles, exact ties, kinds, ignore ------------------------------------------------------------------------------------
def test_obstacles_ties_kinds_and_ignore(ctx):
    gw, obs = _tie_world(ctx)
    T = world_targets(gw, obstacles=obs)
    S = Sweeper(T, obs)
    # bodies 0 and 1 and obstacle 0's component 0 are the same sphere at (0, 5, 0); body 4 and obstacle 1 the same sphere at (8, 5, 0)
    casts = np.concatenate([
        _cast(0, (0, 5.2, 0), (0, 0, 0), 0.2, (0, 0, 0)),        # overlapping bodies 0, 1 and obstacle 0 at t = 0
        _cast(1, (-0.3, 5.1, 0), (0.6, 0, 0), 0.2, (0, 0, 0)),   # the same, a capsule
        _cast(0, (0, 9, 0), (0, 0, 0), 0.3, (0, -6, 0)),         # coming down onto the three (two bodies: one t)
        _cast(1, (8, 9, -0.2), (0, 0, 0.4), 0.3, (0, -6, 0)),    # onto body 4 and obstacle 1
        _cast(0, (0, 0.5, 6), (0, 0, 0), 0.5, (0, 0, 0)),        # inside obstacle 0's component 1 only
        _cast(1, (0, 9, 6), (0.5, 0, 0), 0.4, (0, -9, 0)),       # down onto obstacle 0's component 1
        _cast(0, (4, 9, 0), (0, 0, 0), 0.3, (0, -8, 0)),         # onto the capsule body 2
        _cast(1, (-4, 9, 0.3), (0, 0, 0.5), 0.2, (0, -9, 0)),    # onto body 3
        _cast(0, (30, 30, 30), (0, 0, 0), 0.5, (1, 1, 1)),       # nothing
    ])
    for kinds in range(1, 8):
        compare_sweeps(gw, S, casts, kinds=kinds)
    got = gw.sweep(casts)
    # exact ties at t = 0 go to the body with the smaller caller index, then to the obstacle's component with the smaller index
    assert (got[0]["kind"], got[0]["index"], got[0]["t"]) == (0, 0, 0.0) and (got[1]["kind"], got[1]["index"]) == (0, 0)
    got = gw.sweep(casts, kinds=1)
    assert (got[2]["kind"], got[2]["index"]) == (0, 0) and (got[3]["kind"], got[3]["index"]) == (0, 4)
    got = gw.sweep(casts, kinds=4)
    assert (got[0]["kind"], got[0]["index"], got[0]["part"], got[0]["t"]) == (2, 0, 0, 0.0)
    assert (got[4]["kind"], got[4]["index"], got[4]["part"]) == (2, 0, 1) and (got[5]["index"], got[5]["part"]) == (0, 1)
    assert got[3]["kind"] == 2 and got[3]["index"] == 1
    got = gw.sweep(casts[:1], kinds=5)
    assert got[0]["kind"] == 0  # the body before the obstacle at the same t
    # ignore: the caster's own body is skipped, every part of it
    ign = np.array([0, 1, 0, 4, -1, -1, 2, 3, 0], np.int32)
    compare_sweeps(gw, S, casts, ignore=ign)
    got = gw.sweep(casts[:1], ignore=[0])
    assert got[0]["kind"] == 0 and got[0]["index"] == 1 and got[0]["t"] == 0.0
    assert gw.sweep(casts[8:], ignore=[-1])[0]["kind"] == -1


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
    S = Sweeper(T, obs)
    shp = gw.colliders()
    rng = np.random.default_rng(14)
    aim = np.concatenate([shp["p"], np.array([[0.4, 0.6, -0.3], [-1.0, 0.5, 1.5], [1.5, 0.5, 1.5]], np.float32)])
    casts = casts_at(rng, aim, 96, 1.0, (0.0, 4.0))
    for kinds in (7, 4, 6):
        got, _, _ = compare_sweeps(gw, S, casts, kinds=kinds)
    assert np.any(got["kind"] == 2)


# ---- a re-sorted store, a runaway body, a cast wider than a cell --------------------------------------------------------------
def test_resorted_store_reports_caller_indices(ctx):
    sc = scenes.sphere_pile(12, 6, 12)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 70)  # past the store's re-sort at 64 ticks
    T = world_targets(gw, sc)
    S = Sweeper(T)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(15)
    casts = casts_at(rng, cen, 128, 0.4, (0.0, 8.0))
    got, hits, _ = compare_sweeps(gw, S, casts)
    assert hits > 64


def test_a_runaway_body_and_a_cast_wider_than_a_cell(ctx):
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
    S = Sweeper(T)
    cen = comps["p"][:-1]
    rng = np.random.default_rng(16)
    casts = casts_at(rng, cen, 96, 0.4, (0.0, 30.0))
    up = casts_at(rng, cen, 32, 0.4, (0.0, 0.0))  # from above the pile straight up to the runaway body
    up["p"][:, 1] = cen[:, 1].max() + 2.0 - 0.5 * up["d"][:, 1]
    up["delta"] = (0.0, 30.0, 0.0)
    got, _, _ = compare_sweeps(gw, S, np.concatenate([casts, up]))
    assert np.any(got["index"] == n - 1)
    assert gw.counter("query_large_bodies") >= 1
    # casts far wider than a cell: a sphere of radius 3, a capsule 10 long and 2.5 thick, one that spans the whole grid
    wide = np.concatenate([_cast(0, cen[5] + (0, 8, 0), (0, 0, 0), 3.0, (0, -10, 0)),
                           _cast(1, cen[9] + (-5, 6, 0), (10, 0, 0), 2.5, (0.5, -9, 0.5)),
                           _cast(1, (-40, cen[0][1], 0), (80, 0, 0), 1.2, (0, 0, 0)),
                           _cast(0, cen[3] + (-20, 0, -20), (0, 0, 0), 1.6, (40, 0.5, 40))])
    got, hits, _ = compare_sweeps(gw, S, wide)
    assert hits == 4


# ---- a tile set: ghosts are not reported ---------------------------------------------------------------------------------------
def test_ghosts_are_never_reported(ctx):
    import torch
    sc = scenes.sphere_pile(8, 4, 8)
    n = len(sc["comps"])
    dt = float(sc["dt"])
    gw = mgf_amd.World.from_scene(ctx, sc)
    other = mgf_amd.World.from_scene(ctx, sc)
    other.begin_tick(dt)
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    recs = torch.zeros((n, 72), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    other.export_bodies(ids.data_ptr(), n, recs.data_ptr())
    gw.begin_tick(dt)
    gw.import_ghosts(recs.data_ptr(), n)
    assert gw.ghost_len() == n and len(gw) == n
    T = world_targets(gw, sc)
    S = Sweeper(T)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(17)
    casts = casts_at(rng, cen, 64, 0.4, (0.0, 5.0))
    got, hits, _ = compare_sweeps(gw, S, casts)
    assert hits > 0 and got["index"].max() < n
    torch.cuda.synchronize()


# ---- sweeps do not disturb the tick --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [False, True])
def test_sweeps_leave_the_tick_bit_identical(ctx, many):
    sc = scenes.sphere_pile(10, 6, 10)
    a, b = mgf_amd.World.from_scene(ctx, sc), mgf_amd.World.from_scene(ctx, sc)
    for w in (a, b):
        w.set_option("resort_every", 2)
    dt, iters = float(sc["dt"]), sc["iters"]
    rng = np.random.default_rng(18)
    for k in range(5 if many else 10):
        if many:
            a.step_many(dt, iters, 2)
            b.step_many(dt, iters, 2)
        else:
            a.step(dt, iters)
            b.step(dt, iters)
        a.sweep(casts_at(rng, a.colliders()["p"], 64, 0.5, (0.0, 6.0)))
    sa, sb = a.state(), b.state()
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]).view(np.uint32), np.asarray(sb[key]).view(np.uint32)), key
    ca, cb = a.constraints(), b.constraints()
    assert len(ca) == len(cb) > 0 and ca.tobytes() == cb.tobytes()


# ---- empty ----------------------------------------------------------------------------------------------------------------------
def test_an_empty_world_and_no_casts(ctx):
    gw = mgf_amd.World(ctx)
    casts = np.concatenate([_cast(0, (0, 0, 0), (0, 0, 0), 0.5, (1, 0, 0)), _cast(1, (0, 0, 0), (1, 0, 0), 0.5, (0, 0, 0))])
    got = gw.sweep(casts)
    assert np.all(got["kind"] == -1) and not np.any(got["index"]) and not np.any(got["part"]) and not np.any(got["t"])
    sc = scenes.sphere_pile(4, 2, 4)
    gw = mgf_amd.World.from_scene(ctx, sc)
    assert len(gw.sweep(np.zeros(0, mgf_amd.MOVING_DTYPE))) == 0
    # COMPONENT_DTYPE rows with one delta for all
    rows = np.zeros(2, scenes.COMPONENT_DTYPE)
    rows["r"] = 0.3
    rows["p"] = gw.colliders()["p"][:2] + np.array([0, 3, 0], np.float32)
    T = world_targets(gw, sc)
    got = gw.sweep(rows, (0.0, -4.0, 0.0))
    casts = np.zeros(2, mgf_amd.MOVING_DTYPE)
    for k in ("tag", "p", "d", "r"):
        casts[k] = rows[k]
    casts["delta"] = (0.0, -4.0, 0.0)
    assert got.tobytes() == gw.sweep(casts).tobytes()
    compare_sweeps(gw, Sweeper(T), casts)


# ---- full size once ----------------------------------------------------------------------------------------------------------
def test_config_2_full_size(ctx):
    sc = scenes.config(1)
    gw = mgf_amd.World.from_scene(ctx, sc)
    gw.step_many(float(sc["dt"]), sc["iters"], 3)
    T = world_targets(gw, sc)
    S = Sweeper(T)
    cen = gw.colliders()["p"]
    rng = np.random.default_rng(19)
    n = 65536
    casts = casts_at(rng, cen, n, 1.0, (0.0, 6.0))
    casts["delta"][: n // 8] *= 0.0
    got, hits, _ = compare_sweeps(gw, S, casts)
    assert hits > n // 2
