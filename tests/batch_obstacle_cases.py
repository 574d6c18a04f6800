"""The compounds, worlds, rays and casts of tests/test_gpu_world_batch_obstacles.py (a batch whose worlds have static Compound obstacles
of their own), shared with the CPU check of their conditions (tests/test_world_batch_obstacles_host.py): built here so that both see
the same inputs."""
import numpy as np

from mgf_amd import scenes
from mgf_amd._capi import MOVING_DTYPE
from oracle import oracle as O
from tests import batch_query_cases as BQ
from tests.util import oracle_world

f32 = np.float32
TICKS = 40                      # of the free run; the queries follow it
LIST_TICKS = (1, 2, 20, 30, 40)
RAY_SEED = 311
N_RAYS, N_CASTS = 28, 18        # per world, ahead of the tie cases
# the worlds (the issue's 1 .. 7 at 0 .. 6)
BOX, FIELD, BARE, POSED, PLAIN, EMPTY, HOLE = range(7)


def _quat(axis, angle):
    """a unit quaternion (s, x, y, z) in f32, normalised in f64 first (mgf_compound_set_pose takes it as normalised)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    q = np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * a])
    return tuple(float(v) for v in (q / np.linalg.norm(q)).astype(f32))


IDENT = (1.0, 0.0, 0.0, 0.0)


def compounds():
    """a rotated ramp of three capsules with a ball on its end (a tree deeper than one level), a ring of ten spheres, a single sphere (a
    tree of one leaf) and an empty compound"""
    ramp = np.zeros(4, scenes.COMPONENT_DTYPE)
    ramp["tag"] = [1, 1, 1, 0]
    ramp["p"] = [(-3.0, 0.4, -1.0), (-3.0, 0.4, 0.0), (-3.0, 0.4, 1.0), (3.2, 0.9, 0.0)]
    ramp["d"] = [(6.0, 1.0, 0.0), (6.0, 1.0, 0.0), (6.0, 1.0, 0.0), (0, 0, 0)]
    ramp["r"] = [0.35, 0.35, 0.35, 0.8]
    k = 10
    ang = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
    ring = np.zeros(k, scenes.COMPONENT_DTYPE)
    ring["p"] = np.stack([2.5 * np.cos(ang), np.full(k, 0.5), 2.5 * np.sin(ang)], axis=1)
    ring["r"] = 0.55
    single = np.zeros(1, scenes.COMPONENT_DTYPE)
    single["p"], single["r"] = (0.0, 0.0, 0.0), 0.8
    return dict(ramp=ramp, ring=ring, single=single, empty=np.zeros(0, scenes.COMPONENT_DTYPE))


def obstacle_scenes():
    """0 spheres in a box with ramp + ring; 1 capsules and spheres over a heightfield with ring + ramp (the other order), both turned;
    2 spheres without terrain falling onto the ring; 3 world 0's scene with the same two entries at other poses (the geometry shared, the
    pose not); 4 world 0's scene without obstacles; 5 no bodies, with obstacles - the ring twice at one pose, so that whatever meets it is
    an exact tie between two list entries; 6 a world whose list is (empty compound, single sphere)"""
    C = compounds()
    box = scenes.sphere_pile(4, 3, 4)
    field = scenes.capsule_field_dense(3, 2, 3, sphere_fraction=0.4)
    ramp0 = (C["ramp"], (0.4, 0.2, -0.3), _quat((0, 1, 0), 0.4))
    ring0 = (C["ring"], (-0.3, 0.0, 0.4), IDENT)
    ring1 = (C["ring"], (0.1, 0.05, -0.1), IDENT)
    return [
        dict(box, obstacles=[ramp0, ring0]),
        dict(field, obstacles=[(C["ring"], (0.3, 0.4, -0.2), _quat((1, 0, 0.2), 0.3)), (C["ramp"], (0.0, 0.3, 0.5), _quat((0.1, 1, 0), -0.7))]),
        dict(scenes.sphere_pile(6, 1, 6, seed=11), terrain=None, obstacles=[(C["ring"], (0.2, -1.2, 0.1), IDENT)]),
        dict(box, obstacles=[(C["ramp"], (-0.5, 0.35, 0.4), _quat((0, 1, 0), -0.9)), (C["ring"], (0.8, 0.1, -1.0), _quat((0, 0, 1), 0.15))]),
        dict(box, obstacles=[]),
        dict(BQ.empty_scene(box["terrain"]), obstacles=[ramp0, ring1, ring1]),
        dict(scenes.sphere_pile(2, 2, 2, seed=3), obstacles=[(C["empty"], (0.0, 1.0, 0.0), IDENT), (C["single"], (0.2, 0.3, 0.1), _quat((1, 1, 0), 0.5))]),
    ]


def oracle_with_obstacles(sc, obstacles=None):
    """the oracle world of the scene, add_obstacle called once per entry of its list, in list order"""
    ow = oracle_world(sc)
    for comps, disp, rot in (sc["obstacles"] if obstacles is None else obstacles):
        ow.add_obstacle(comps, disp, rot)
    return ow


def oracle_compounds(obstacles):
    out = []
    for comps, disp, rot in obstacles:
        c = O.Compound([O.component(int(r["tag"]), r["p"], r["d"], float(r["r"])) for r in comps])
        c.set_pose(disp, rot)
        out.append(c)
    return out


def obstacle_contacts(ow, compounds_):
    """per body of the oracle world, per obstacle: the contacts Compound.contacts reports for the collider and motion of its last tick"""
    comps, delta = ow.colliders()
    out = []
    for r, d in zip(comps, delta):
        sh = O.shape(O.SPHERE, r["p"], float(r["r"])) if r["tag"] == 0 else O.shape(O.CAPSULE, r["p"], r["d"], float(r["r"]))
        out.append([len(c.contacts(sh, d)) for c in compounds_])
    return np.array(out, np.int64).reshape(len(comps), len(compounds_))


def _rotate(q, v):
    s, u = q[0], np.asarray(q[1:], np.float64)
    v = np.asarray(v, np.float64)
    return v + 2.0 * np.cross(u, np.cross(u, v) + s * v)


def component_centres(obstacles):
    """about where every component of every list entry is in the world (to aim at)"""
    out = []
    for comps, disp, rot in obstacles:
        for r in comps:
            mid = r["p"].astype(np.float64) + 0.5 * r["d"].astype(np.float64) * (r["tag"] == 1)
            out.append(_rotate(rot, mid) + np.asarray(disp, np.float64))
    return np.array(out).reshape(-1, 3)


def centres_of(comps):
    return (np.asarray(comps["p"], f32) + f32(0.5) * np.asarray(comps["d"], f32) * (comps["tag"] == 1)[:, None]).astype(f32)


def rays_and_casts(scs, centres):
    """Per world N_RAYS particles and N_CASTS casts, then the tie cases, all in one seeded shuffle each.  The particles: three in five aimed at
    a component of an obstacle from above or from the side, one in five at a body, the rest along the floor from outside (the terrain, or a
    body or an obstacle in front of it) and straight up (nothing); every other one a segment; some ignore the body they aim at.  The
    casts: spheres and capsules alternating, dropped onto a component or a body; cast 1 of a world a sphere that does not move, inside a
    component.  The ties: in the world whose list holds the ring twice at one pose, particles and casts straight down onto ring spheres -
    the two list entries answer with the same t, bit for bit, and the first wins."""
    rng = np.random.default_rng(RAY_SEED)
    RW, RP, RD, RT, RI, CW, CC = [], [], [], [], [], [], []
    for k, sc in enumerate(scs):
        oc = component_centres(sc["obstacles"])
        bc = np.asarray(centres[k], np.float64).reshape(-1, 3)
        p, d = np.zeros((N_RAYS, 3)), np.zeros((N_RAYS, 3))
        dt, ign = np.full(N_RAYS, np.inf), np.full(N_RAYS, -1, np.int64)
        for i in range(N_RAYS):
            kind = (0, 0, 1, 0, 2)[i % 5]
            if kind == 0 and len(oc):
                tgt = oc[rng.integers(0, len(oc))] + rng.normal(0, 0.15, 3)
                p[i] = tgt + ((rng.normal(0, 1.0), 12.0 + rng.uniform(0, 3), rng.normal(0, 1.0)) if i % 2 else (9.0 * rng.choice([-1.0, 1.0]), rng.uniform(0, 1.0), rng.normal(0, 1.0)))
                d[i] = tgt - p[i]
            elif kind == 1 and len(bc):
                j = int(rng.integers(0, len(bc)))
                tgt = bc[j] + rng.normal(0, 0.2, 3)
                p[i] = (tgt[0] + rng.normal(0, 1.5), 14.0 + rng.uniform(0, 3), tgt[2] + rng.normal(0, 1.5))
                d[i] = tgt - p[i]
                if i % 4 == 1:
                    ign[i] = j
            elif i % 2:
                p[i] = (0.1 * i, 20.0, 0.3)
                d[i] = (0.0, 1.0, 0.0)
            else:
                p[i] = (-9.0, 0.25 + 0.02 * i, rng.uniform(-2.0, 2.0))
                d[i] = (1.0, 0.0, 0.0)
            if i % 2 == 0 and kind != 2:
                dt[i] = 1.0
                d[i] *= rng.uniform(0.6, 1.6)
        RW.append(np.full(N_RAYS, k, np.int32)); RP.append(p); RD.append(d); RT.append(dt); RI.append(ign)
        c = np.zeros(N_CASTS, MOVING_DTYPE)
        c["tag"] = np.arange(N_CASTS) % 2
        c["r"] = rng.uniform(0.15, 0.4, N_CASTS)
        ax = rng.normal(0, 1, (N_CASTS, 3))
        ax *= (rng.uniform(0.3, 0.9, N_CASTS) / np.linalg.norm(ax, axis=1))[:, None]
        c["d"] = np.where((c["tag"] == 1)[:, None], ax, 0.0)
        for i in range(N_CASTS):
            pool = oc if (i % 4 != 3 and len(oc)) or not len(bc) else bc
            tgt = (pool[rng.integers(0, len(pool))] if len(pool) else np.zeros(3)) + rng.normal(0, 0.2, 3)
            src = tgt + (rng.normal(0, 0.5), 4.0 + rng.uniform(0, 3), rng.normal(0, 0.5))
            c["p"][i] = src - 0.5 * c["d"][i]
            c["delta"][i] = (tgt - src) * rng.uniform(0.7, 1.5)
        if len(oc):
            c["tag"][1], c["p"][1], c["d"][1], c["r"][1], c["delta"][1] = 0, oc[-1] + (0.05, 0.02, 0.0), (0, 0, 0), 0.2, (0, 0, 0)
        CW.append(np.full(N_CASTS, k, np.int32)); CC.append(c)
    # the ties: onto the doubled ring of the world without bodies
    ring = component_centres(scs[EMPTY]["obstacles"][1:2])
    tp = np.array([ring[0] + (0.0, 6.0, 0.0), ring[3] + (0.1, 7.0, -0.05), ring[7] + (-0.05, 5.0, 0.1)])
    RW.append(np.full(3, EMPTY, np.int32)); RP.append(tp); RD.append(np.tile([0.0, -1.0, 0.0], (3, 1))); RT.append(np.full(3, np.inf)); RI.append(np.full(3, -1))
    tc = np.zeros(3, MOVING_DTYPE)
    tc["tag"] = [0, 1, 0]
    tc["r"] = [0.3, 0.25, 0.2]
    tc["d"] = [(0, 0, 0), (0.4, 0.0, 0.1), (0, 0, 0)]
    tc["p"] = [ring[1] + (0.0, 4.0, 0.0), ring[5] + (-0.2, 5.0, 0.0), ring[8] + (0.02, 0.1, 0.0)]
    tc["delta"] = [(0, -6.0, 0), (0, -7.0, 0), (0, 0, 0)]
    CW.append(np.full(3, EMPTY, np.int32)); CC.append(tc)
    rays = dict(world=np.concatenate(RW), p=np.concatenate(RP).astype(f32), d=np.concatenate(RD).astype(f32), dt=np.concatenate(RT).astype(f32),
                ignore=np.concatenate(RI).astype(np.int32))
    n = len(rays["world"])
    tie = np.zeros(n, bool)
    tie[-3:] = True
    perm = rng.permutation(n)
    rays = {k: v[perm] for k, v in rays.items()}
    rays["tie"] = tie[perm]
    cw, casts = np.concatenate(CW), np.concatenate(CC)
    ctie = np.zeros(len(cw), bool)
    ctie[-3:] = True
    perm = rng.permutation(len(cw))
    return rays, dict(world=cw[perm], casts=casts[perm], tie=ctie[perm])


def world_faces(sc):
    t = sc["terrain"]
    if t is None:
        return None
    v = np.asarray(t["verts"], f32).reshape(-1, 3) + np.asarray(t["pos"], f32)
    return v[np.asarray(t["faces"], np.int64).reshape(-1, 3)]
