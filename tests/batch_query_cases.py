"""The scenes and the rays of tests/test_gpu_world_batch_queries.py, shared with the CPU check of their conditions
(tests/test_world_batch_query_host.py): built here so that both see the same queries."""
import numpy as np

from mgf_amd import scenes

RAY_SEED = 20
COUNTS_T0 = (3, 64, 257, 1, 300)    # rays per world at tick 0 ...
COUNTS_T30 = (3, 64, 300, 0, 257)   # ... and after 30 ticks: 0, 1, 3, 64, 257 and 300 all occur


def empty_scene(terrain):
    sc = scenes.sphere_pile(1, 1, 1)
    return dict(sc, name="empty", comps=sc["comps"][:0], mass=sc["mass"][:0], restitution=sc["restitution"][:0], friction=sc["friction"][:0],
                force=sc["force"][:0], v0=None, terrain=terrain)


def pile_scenes():
    """1, 96, 512, 0 and 1024 spheres (the LDS maximum) over the largest scene's box"""
    big = scenes.sphere_pile(8, 16, 8)
    out = [scenes.sphere_pile(1, 1, 1), scenes.sphere_pile(4, 6, 4, seed=5), scenes.sphere_pile(8, 8, 8), None, big]
    out[3] = empty_scene(big["terrain"])
    return [dict(sc, terrain=big["terrain"]) for sc in out]


def pile_rays(centres, counts, seed=RAY_SEED):
    """counts[k] particles for world k whose bodies' centres are centres[k], in one interleaved order (a seeded shuffle).  Per world:
    first a ray straight down at body 0 (a body), one pointing up (nothing), one from outside the box along the floor (the wall: terrain);
    then rays aimed at (near) a body's centre, 70 % from above the open box and 30 % from outside its walls, half of them rays (dt = inf)
    and half segments (dt = 1) of 0.5 .. 1.5 times the distance; every 16th has d = 0; a third ignore the body they are aimed at."""
    rng = np.random.default_rng(seed)
    W, P, D, DT, IGN = [], [], [], [], []
    for k, (cen, c) in enumerate(zip(centres, counts)):
        cen = np.asarray(cen, np.float64).reshape(-1, 3)
        p = np.zeros((c, 3))
        d = np.zeros((c, 3))
        dt = np.full(c, np.inf)
        ign = np.full(c, -1, np.int64)
        for i in range(c):
            if len(cen) == 0 or i == 2 or (c == 1):
                p[i] = (-9.0, 0.3 + 0.01 * i, 0.2)            # outside the box, along the floor: the wall
                d[i] = (1.0, 0.0, 0.0)
            elif i == 0:
                p[i] = cen[0] + (0.0, 25.0, 0.0)              # straight down at body 0
                d[i] = (0.0, -1.0, 0.0)
            elif i == 1:
                p[i] = cen[0] + (0.1, 25.0, 0.0)              # up and away
                d[i] = (0.0, 1.0, 0.0)
            else:
                j = int(rng.integers(0, len(cen)))
                tgt = cen[j] + rng.normal(0.0, 0.25, 3)
                if rng.random() < 0.7:
                    p[i] = (tgt[0] + rng.normal(0, 2.0), 22.0 + rng.uniform(0, 4.0), tgt[2] + rng.normal(0, 2.0))
                else:
                    side = 1.0 if rng.random() < 0.5 else -1.0
                    p[i] = (side * (8.0 + rng.uniform(0, 3.0)), tgt[1] + rng.normal(0, 1.0), tgt[2] + rng.normal(0, 2.0))
                d[i] = tgt - p[i]
                if i % 2:
                    dt[i] = 1.0
                    d[i] *= rng.uniform(0.5, 1.5)
                if i % 16 == 5:
                    d[i] = 0.0
                if i % 3 == 0:
                    ign[i] = j
        W.append(np.full(c, k, np.int32)); P.append(p); D.append(d); DT.append(dt); IGN.append(ign)
    W, P, D, DT, IGN = (np.concatenate(a) for a in (W, P, D, DT, IGN))
    perm = rng.permutation(len(W))
    return dict(world=W[perm], p=P[perm].astype(np.float32), d=D[perm].astype(np.float32), dt=DT[perm].astype(np.float32), ignore=IGN[perm].astype(np.int32))
