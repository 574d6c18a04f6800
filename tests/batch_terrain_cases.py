"""The scenes, rays and casts of tests/test_gpu_world_batch_terrains.py (a batch whose worlds have terrains of their own), shared with
the CPU check of their conditions (tests/test_world_batch_terrains_host.py): built here so that both see the same inputs."""
import numpy as np

from mgf_amd import scenes
from mgf_amd._capi import MOVING_DTYPE
from tests import batch_query_cases as BQ
from tests.util import oracle_world

f32 = np.float32
TICKS = 40                      # of the free run; the queries follow it
LIST_TICKS = (1, 2, 20, 30, 40)
OTHER_SEED = 4242               # the second heightfield (and its capsules)
RAISE = 0.3                     # the twin's terrain is this much higher: not a representable number
RAY_COUNTS = (40, 40, 40, 40, 20, 3)
RAY_SEED = 77
PROBES = 7                      # a PROBES x PROBES grid of rays straight down, the same in every world
HEIGHTFIELDS = (0, 1)           # the two worlds over different heightfields
TWINS = (0, 3)                  # the same scene, the terrain of the second raised
BARE, EMPTY = 4, 5


def mixed_scenes():
    """a heightfield with capsules; another heightfield with other capsules; spheres in a box; the first again over its terrain raised by
    0.3 (the geometry shared, the position not); spheres without terrain; no bodies in the box"""
    a = scenes.capsule_field(4, 3, 4)
    b = scenes.capsule_field(4, 3, 4, seed=OTHER_SEED)
    c = scenes.sphere_pile(4, 6, 4, seed=5)
    raised = dict(a["terrain"], pos=(np.asarray(a["terrain"]["pos"], f32) + f32([0.0, RAISE, 0.0])).astype(f32))
    return [a, b, c, dict(a, terrain=raised), dict(scenes.sphere_pile(3, 3, 3), terrain=None), BQ.empty_scene(c["terrain"])]


def small_scenes():
    """three small worlds for a batch that cycles over them: spheres in a box, capsules over a heightfield, spheres over that heightfield raised"""
    a = scenes.sphere_pile(3, 3, 3)
    h = scenes.capsule_field(2, 2, 2, seed=9)
    raised = dict(h["terrain"], pos=f32([0.0, RAISE, 0.0]))
    return [a, h, dict(scenes.sphere_pile(2, 3, 2, seed=3), terrain=raised)]


def run_oracles(scs, ticks):
    """one oracle world per scene through `ticks` ticks -> the worlds and, per world and tick, (n_constraints, n_terrain_constraints)"""
    ows = [oracle_world(sc) for sc in scs]
    stats = []
    for ow, sc in zip(ows, scs):
        stats.append([])
        for _ in range(ticks):
            st = ow.step(float(sc["dt"]), sc["iters"])   # (the oracle world hands out one record: copy what is kept)
            stats[-1].append((int(st.n_constraints), int(st.n_terrain_constraints)))
    return ows, stats


def centres_of(comps):
    """the middle of every collider (COMPONENT / MOVING rows)"""
    return (np.asarray(comps["p"], f32) + f32(0.5) * np.asarray(comps["d"], f32) * (comps["tag"] == 1)[:, None]).astype(f32)


def mixed_rays(centres):
    """batch_query_cases.pile_rays' scheme for RAY_COUNTS particles per world, and in every world the same PROBES x PROBES grid of rays
    straight down from y = 30 over [-8, 8]^2 (beyond every terrain's edge: those meet nothing), all in one seeded shuffle"""
    base = BQ.pile_rays(centres, RAY_COUNTS, seed=RAY_SEED)
    g = np.linspace(-8.0, 8.0, PROBES)
    X, Z = np.meshgrid(g, g, indexing="ij")
    pp = np.stack([X.ravel(), np.full(X.size, 30.0), Z.ravel()], axis=1).astype(f32)
    K, n = len(centres), len(pp)
    probe = dict(world=np.repeat(np.arange(K, dtype=np.int32), n), p=np.tile(pp, (K, 1)), d=np.tile(f32([0.0, -1.0, 0.0]), (K * n, 1)),
                 dt=np.full(K * n, np.inf, f32), ignore=np.full(K * n, -1, np.int32))
    probe_id = np.concatenate([np.full(len(base["world"]), -1), np.tile(np.arange(n), K)])
    perm = np.random.default_rng(RAY_SEED + 1).permutation(len(probe_id))
    out = {k: np.concatenate([base[k], probe[k]])[perm] for k in base}
    out["probe"] = probe_id[perm]   # the probe's place in the grid, -1 for a ray of pile_rays'
    return out


def mixed_casts(centres):
    """per world 24 casts - spheres and capsules alternating - from above its bodies (above the origin for a world without any) down
    and sideways through them into the ground; cast 0 a capsule that does not move and lies in the ground - its lower side at y = -0.3, below every terrain here - (every face is
    tested),
    cast 1 a sphere with delta = 0 at a body (at the ground for a world without any); one seeded shuffle -> (world, casts)"""
    rng = np.random.default_rng(RAY_SEED + 2)
    W, C = [], []
    for k, cen in enumerate(centres):
        n = 24
        cen = np.asarray(cen, np.float64).reshape(-1, 3)
        at = cen[rng.integers(0, len(cen), n)] if len(cen) else np.zeros((n, 3))
        c = np.zeros(n, MOVING_DTYPE)
        c["tag"] = np.arange(n) % 2
        c["r"] = rng.uniform(0.2, 0.5, n)
        ax = rng.normal(0, 1, (n, 3))
        ax *= (rng.uniform(0.3, 1.2, n) / np.linalg.norm(ax, axis=1))[:, None]
        c["d"] = np.where((c["tag"] == 1)[:, None], ax, 0.0)
        src = at + rng.normal(0, 0.5, (n, 3)) + np.array([0.0, 3.0, 0.0])
        c["p"] = src - 0.5 * c["d"]
        c["delta"] = rng.normal(0, 0.6, (n, 3)) + np.array([0.0, -1.0, 0.0]) * rng.uniform(1.0, 8.0, (n, 1))
        low = at[0] * np.array([1.0, 0.0, 1.0])
        for i, (tag, p, d, r) in enumerate(((1, low + (0.0, 0.2, 0.0), (0.6, 0.05, 0.1), 0.5),
                                            (0, (at[1] if len(cen) else low) + (0.05, 0.02, 0.0), (0.0, 0.0, 0.0), 0.3))):
            c["tag"][i], c["p"][i], c["d"][i], c["r"][i], c["delta"][i] = tag, p, d, r, (0.0, 0.0, 0.0)
        W.append(np.full(n, k, np.int32))
        C.append(c)
    W, C = np.concatenate(W), np.concatenate(C)
    perm = rng.permutation(len(W))
    return W[perm], C[perm]


def world_faces(sc):
    """the scene's terrain faces in world coordinates (F, 3, 3), None without terrain"""
    t = sc["terrain"]
    if t is None:
        return None
    v = np.asarray(t["verts"], f32).reshape(-1, 3) + np.asarray(t["pos"], f32)
    return v[np.asarray(t["faces"], np.int64).reshape(-1, 3)]
