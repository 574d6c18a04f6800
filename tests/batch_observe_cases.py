"""The scenes, the boxes and the expected-value arithmetic of tests/test_gpu_world_batch_observe.py, shared with the CPU check of their
conditions (tests/test_world_batch_observe_host.py): built here so that both see the same inputs."""
import numpy as np

from mgf_amd import scenes
from mgf_amd._capi import BODY_CONTACTS_DTYPE

f32 = np.float32
BOX_SEED = 41
HUB_R, HUB_r, HUB_N = 3.0, 0.2, 300


def hub_scene(hub_first):
    """One sphere of R = 3 at (0, 10, 0) and 300 spheres of r = 0.2 on a Fibonacci sphere around it, their centres R + r - 0.02 from its
    centre, moving inward at 2 m/s; no terrain.  hub_first: the hub is body 0 (it is `b` of 300 records); else it is the last body (its
    own range of the list is 300 records long).  The smallest case in which one body's chain crosses the 256 lanes of a workgroup."""
    i = np.arange(HUB_N, dtype=np.float64)
    y = 1.0 - 2.0 * (i + 0.5) / HUB_N
    rad = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([rad * np.cos(phi), y, rad * np.sin(phi)], axis=1)
    centre = np.array([0.0, 10.0, 0.0])
    small = centre + u * (HUB_R + HUB_r - 0.02)
    c = np.concatenate([centre[None], small] if hub_first else [small, centre[None]]).astype(f32)
    r = np.full(HUB_N + 1, HUB_r, f32)
    v0 = np.zeros((HUB_N + 1, 3), f32)
    hub = 0 if hub_first else HUB_N
    r[hub] = HUB_R
    rest = np.arange(HUB_N + 1) != hub
    v0[rest] = (-2.0 * u).astype(f32)
    sc = scenes.sphere_pile(1, 1, 1)
    n = HUB_N + 1
    comps = np.zeros(n, scenes.COMPONENT_DTYPE)
    comps["p"], comps["r"] = c, r
    return dict(sc, name="hub_first" if hub_first else "hub_last", comps=comps, mass=np.full(n, 1.0, f32), restitution=np.full(n, 0.3, f32),
                friction=np.full(n, 0.6, f32), force=np.tile(f32([0.0, -9.8, 0.0]), (n, 1)), v0=v0, terrain=None), hub


def capsule_scenes():
    """the two worlds of test_capsules_and_a_heightfield (tests/test_gpu_world_batch.py): 48 capsules, and 256 capsules and spheres, over one heightfield"""
    a, c = scenes.capsule_field(4, 3, 4), scenes.capsule_field(8, 4, 8, sphere_fraction=0.5)
    return [a, dict(c, terrain=a["terrain"])]


def fold(cons, n):
    """mgf_body_contacts of a world of n bodies from its constraint list (CONSTRAINT_DTYPE rows, insertion order), as include/mgf_hip.h
    defines it: per body its own range of the list first (the body is `a`), then the records where it is `b`, ascending; sequential f32
    operations: t = normal * ni; impulse -= t as `a`, impulse += t as `b`; normal_impulse += ni."""
    out = np.zeros(n, BODY_CONTACTS_DTYPE)
    own = [[] for _ in range(n)]
    asb = [[] for _ in range(n)]
    for c, (a, b) in enumerate(zip(cons["a"].tolist(), cons["b"].tolist())):
        own[a].append(c)
        if b >= 0:
            asb[b].append(c)
    normal = np.ascontiguousarray(cons["normal"], f32)
    ni = np.ascontiguousarray(cons["normal_impulse"], f32)
    for x in range(n):
        imp = np.zeros(3, f32)
        s = f32(0.0)
        for c in own[x]:
            t = normal[c] * ni[c]
            imp = imp - t
            s = f32(s + ni[c])
        for c in asb[x]:
            t = normal[c] * ni[c]
            imp = imp + t
            s = f32(s + ni[c])
        assert imp.dtype == f32
        out[x] = (len(own[x]) + len(asb[x]), sum(1 for c in own[x] if cons["b"][c] < 0), imp, s)
    return out


def categories(cons, n):
    """(records, bodies in a record, records against terrain, bodies that occur as `b`, bodies in no record)"""
    a, b = cons["a"], cons["b"]
    touched = np.zeros(n, bool)
    touched[a] = True
    touched[b[b >= 0]] = True
    return len(cons), int(touched.sum()), int(np.sum(b < 0)), len(np.unique(b[b >= 0])), int(n - touched.sum())


def tight_boxes(col):
    """BoundedBy<AABB> (bounds.rs:170-190) of MOVING_DTYPE / COMPONENT_DTYPE colliders, in f32: (n, 6) rows c.xyz, r.xyz"""
    from tests.test_gpu_world_queries import Targets
    comps = np.zeros(len(col), scenes.COMPONENT_DTYPE)
    for k in ("tag", "p", "d", "r"):
        comps[k] = col[k]
    if len(comps) == 0:
        return np.zeros((0, 6), f32)
    return Targets([[c] for c in comps]).boxes()


def overlaps(bx, q):
    """Overlaps<AABB> (collision.rs:22-29) of box q (c.xyz, r.xyz) with every row of bx, in f32: the body indices, ascending"""
    if len(bx) == 0:
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(bx[:, :3] - q[:3]) <= bx[:, 3:] + q[3:], axis=1)
    return np.nonzero(ok)[0]


def mixed_boxes(centres, counts, seed=BOX_SEED):
    """counts[k] boxes for world k whose bodies' centres are centres[k], interleaved by a seeded shuffle: cubes of width 0.3 .. 3 placed
    around body centres (around the origin for a world without bodies), every eighth lifted by 3 .. 8 so that some meet nothing.
    -> (world int32[n], boxes f32[n, 6])"""
    rng = np.random.default_rng(seed)
    W, B = [], []
    for k, (cen, c) in enumerate(zip(centres, counts)):
        cen = np.asarray(cen, np.float64).reshape(-1, 3)
        at = cen[rng.integers(0, len(cen), c)] if len(cen) else np.zeros((c, 3))
        at = at + rng.normal(0.0, 0.5, (c, 3))
        at[::8, 1] += rng.uniform(3.0, 8.0, len(at[::8]))
        half = rng.uniform(0.15, 1.5, (c, 1)) * np.ones((1, 3))
        W.append(np.full(c, k, np.int32))
        B.append(np.concatenate([at, half], axis=1))
    W, B = np.concatenate(W), np.concatenate(B)
    perm = rng.permutation(len(W))
    return W[perm], B[perm].astype(f32)


def special_boxes(bx):
    """for a world with the tight boxes bx: a box that covers them all; one far away; one whose low x face equals body 0's high x face
    in the test's own f32 arithmetic - |c0.x - qc| == r0.x + qr, so it hits: the test is <= - and its nextafter neighbour (it misses
    body 0); a NaN box; a box with a negative half extent around body 0's centre (it still meets body 0: -0.1 + r0 > 0)."""
    lo, hi = (bx[:, :3] - bx[:, 3:]).min(axis=0), (bx[:, :3] + bx[:, 3:]).max(axis=0)
    cover = np.concatenate([(hi + lo) / 2, (hi - lo) / 2 + 1.0])
    far = np.concatenate([hi + 100.0, [1.0, 1.0, 1.0]])
    c0, r0 = bx[0, :3], bx[0, 3:]
    # qr = 0.25; qc the largest f32 for which |c0.x - qc| in f32 is still <= r0.x + qr in f32
    qr = f32(0.25)
    want = f32(r0[0] + qr)
    qc = f32(c0[0] + want)
    for _ in range(64):   # (a few ulps at most)
        nxt = np.nextafter(qc, f32(np.inf))
        if f32(abs(f32(c0[0] - nxt))) <= want:
            qc = nxt
        else:
            break
    while f32(abs(f32(c0[0] - qc))) > want:
        qc = np.nextafter(qc, f32(-np.inf))
    touch = np.array([qc, c0[1], c0[2], qr, qr, qr], f32)
    miss = touch.copy()
    miss[0] = np.nextafter(qc, f32(np.inf))
    nan = np.array([c0[0], np.nan, c0[2], 1.0, 1.0, 1.0], f32)
    neg = np.array([c0[0], c0[1], c0[2], -0.1, -0.1, -0.1], f32)
    return np.stack([cover.astype(f32), far.astype(f32), touch, miss, nan, neg]).astype(f32)
