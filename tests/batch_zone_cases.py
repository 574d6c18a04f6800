"""Shared by the tests of a batch's box zones (mgf_batch_set_zones / _read_zones / _read_zones_dev / _overlap_first_dev), without a GPU:
a numpy restatement of the definition, f32 operation by operation -
    c = x + rotate(q, p)      r = r      (body = -1: c = p)      rotate: tests/batch_sensor_cases.py's, held to the oracle there
and of the record - the full count, the first k of the list, -1 behind them - from a list; and the scenes and rigs of
tests/test_gpu_world_batch_zones.py, built from the scenes alone so that tests/test_world_batch_zones_host.py sees the same zones."""
import numpy as np

from tests import batch_query_cases as BQ
from tests import batch_sensor_cases as SC

f32 = np.float32
IGNORE_SELF = 1
TICKS = 3
KS = (0, 1, 8, 64, 1024)            # 1024 = MGF_BATCH_MAX_BODIES: above every world's length
PERS = (1, 3, 257)                  # boxes a world for mgf_batch_overlap_first_dev: L = 64, 64, and 1 / 64 (two work items)
W5, WE, W1, W300 = 0, 1, 2, 3       # the worlds of zone_scenes() by what they hold
COUNTS = (3, 2, 20, 257)            # zones a world: L = 64; a world without bodies; L = 8; two work items, L = 1 and L = 64


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def boxes(rig, state, lengths):
    """the boxes of a rig (ZONE_DTYPE rows) from state(None) of a batch whose worlds hold `lengths` bodies: rows (c.xyz, r.xyz) of f32"""
    out = np.empty((len(rig), 6), f32)
    out[:, 0:3], out[:, 3:6] = rig["p"], rig["r"]
    on = np.flatnonzero(rig["body"] >= 0)
    if len(on):
        g = SC.offsets(lengths)[rig["world"][on]] + rig["body"][on]
        x = np.ascontiguousarray(state["x"][g], f32).reshape(-1, 3)
        out[on, 0:3] = x + SC.rotate(state["q"][g], rig["p"][on])
    assert out.dtype == f32
    return out


def ignore_of(rig):
    return np.where(rig["flags"] & IGNORE_SELF, rig["body"], -1).astype(np.int32)


def record(lst, k):
    """the 1 + k words of a zone whose list (ascending body indices, self already removed) is lst"""
    out = np.full(1 + k, -1, np.int32)
    out[0] = len(lst)
    m = min(len(lst), k)
    out[1:1 + m] = lst[:m]
    return out


def records(offsets, bodies, ignore, k):
    """[n, 1 + k] from the CSR lists of WorldBatch.overlap_boxes, ignore[i] (-1: none) removed from list i"""
    n = len(offsets) - 1
    out = np.empty((n, 1 + k), np.int32)
    for i in range(n):
        lst = np.asarray(bodies[int(offsets[i]):int(offsets[i + 1])], np.int64)
        out[i] = record(lst[lst != int(ignore[i])], k)
    return out


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
def zone_scenes():
    """worlds of 5, 0, 1 and 300 bodies - SC.twin_scenes() (spheres, every third body a short capsule; 300: more than 256, so several
    trips of every lane split) with a world without bodies put in behind the first; the one-body world sits in the middle"""
    twin = SC.twin_scenes()
    return [twin[0], BQ.empty_scene(twin[0]["terrain"]), twin[1], twin[2]]


def lengths_of(scs):
    return [len(sc["comps"]) for sc in scs]


def initial_state(scs):
    """x and q of every body as mgf_batch_add_bodies leaves them (Component::deconstruct): a sphere at its centre, unturned; a capsule
    at its middle, turned from +y onto its axis by the oracle's quat_from_arc.  For the conditions a test checks without a GPU."""
    import ctypes as C
    from oracle import oracle as O
    xs, qs = [], []
    for sc in scs:
        c = sc["comps"]
        x = c["p"].astype(f32).copy()
        q = np.tile(f32([1, 0, 0, 0]), (len(c), 1))
        for i in np.flatnonzero(c["tag"] == 1):
            d = c["d"][i].astype(f32)
            x[i] = c["p"][i] + d * f32(0.5)
            h = f32(np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
            out = O.Quat()
            O.lib().mgfo_quat_from_arc(C.byref(O.vec3((0.0, float(h), 0.0))), C.byref(O.vec3(d)), C.byref(out))
            q[i] = (out.s, out.x, out.y, out.z)
        xs.append(x); qs.append(q)
    return dict(x=np.concatenate(xs), q=np.concatenate(qs))


# ---- the rig, from the scenes alone -------------------------------------------------------------------------------------------------------
# what a zone of the rig is for
RANDOM, FIXED, OWN_SEEN, OWN_IGNORED, TWIN, COVER, FAR, NAN_P, NAN_R, NEGATIVE = range(10)


def zone_rig(scs, seed=97):
    """(rig, role): ZONE_DTYPE rows, COUNTS[k] for world k, all worlds in one shuffled order.
    The world of 300 (257 zones, two work items): boxes of half extent 0.2 .. 1.6 a little off a body's centre, a third of them seeing
    their own body; boxes fixed in the world inside the pile; a small box at its body's centre that sees the body (count 1) and one that
    ignores it (count 0); two zones on one body; a box over the whole pile (count 300 - more than every k but 1024 - and the LAST of
    its world in rig order: it is the second work item's only zone, so 64 lanes walk its list across every 64-body trip); a box far
    away; NaN in p on a body, NaN in p in the world, NaN in r; negative half extents (-0.1: still meets its own body, a sphere of r 0.5
    or a capsule; and -2: meets nothing).  The world of 5: three zones.  The world of one body: 20.  The world without bodies: two,
    fixed in the world."""
    from mgf_amd._capi import ZONE_DTYPE
    rng = np.random.default_rng(seed)
    rows, role = [], []

    def add(w, body, p, r, flags, what):
        rows.append((w, body, tuple(np.float32(p)), tuple(np.broadcast_to(np.float32(r), (3,))), flags, 0))
        role.append(what)

    def randoms(w, count):
        nb = len(scs[w]["comps"])
        for i in range(count):
            add(w, int(rng.integers(0, nb)), rng.uniform(-0.4, 0.4, 3), rng.uniform(0.2, 1.6, 3), 0 if i % 3 == 0 else IGNORE_SELF, RANDOM)

    def fixed(w, count):
        cen = SC.centres(scs[w])
        lo, hi = (cen.min(axis=0), cen.max(axis=0)) if len(cen) else (np.zeros(3), np.ones(3))
        for _ in range(count):
            add(w, -1, rng.uniform(lo, hi), rng.uniform(0.2, 1.6, 3), 0, FIXED)

    # the world of 300
    nb = len(scs[W300]["comps"])
    sphere = int(np.flatnonzero(scs[W300]["comps"]["tag"] == 0)[17])
    capsule = int(np.flatnonzero(scs[W300]["comps"]["tag"] == 1)[23])
    cen = SC.centres(scs[W300])
    for body in (sphere, capsule):
        add(W300, body, (0, 0, 0), 0.05, 0, OWN_SEEN)
        add(W300, body, (0, 0, 0), 0.05, IGNORE_SELF, OWN_IGNORED)
        add(W300, body, (0, 0, 0), -0.1, 0, NEGATIVE)
    add(W300, sphere, (0, 0, 0), -2.0, 0, NEGATIVE)
    one = int(rng.integers(0, nb))
    add(W300, one, (0.3, 0.0, 0.0), (1.0, 0.4, 1.0), IGNORE_SELF, TWIN)
    add(W300, one, (-0.3, 0.2, 0.0), (0.4, 1.0, 0.4), 0, TWIN)
    add(W300, -1, (cen.max(axis=0) + cen.min(axis=0)) / 2, (cen.max(axis=0) - cen.min(axis=0)) / 2 + 2.0, 0, COVER)
    add(W300, -1, cen.max(axis=0) + 100.0, 1.0, 0, FAR)
    add(W300, int(rng.integers(0, nb)), (0.0, np.nan, 0.0), 1.0, IGNORE_SELF, NAN_P)
    add(W300, -1, (np.nan, 1.0, 0.0), 1.0, 0, NAN_P)
    add(W300, int(rng.integers(0, nb)), (0, 0, 0), (1.0, 1.0, np.nan), 0, NAN_R)
    fixed(W300, 20)
    randoms(W300, COUNTS[W300] - sum(1 for r in rows if r[0] == W300))
    # the world of 5; the world of one body; the world without bodies
    c5 = SC.centres(scs[W5])
    add(W5, 1, (0.1, 0.0, 0.0), 1.2, IGNORE_SELF, RANDOM)
    add(W5, -1, c5.mean(axis=0), 4.0, 0, COVER)
    add(W5, 4, (0, 0, 0), 0.05, 0, OWN_SEEN)
    add(W1, 0, (0, 0, 0), 0.05, 0, OWN_SEEN)
    add(W1, 0, (0, 0, 0), 0.05, IGNORE_SELF, OWN_IGNORED)
    fixed(W1, 4)
    randoms(W1, COUNTS[W1] - 6)
    fixed(WE, COUNTS[WE])
    rig = np.array(rows, ZONE_DTYPE)
    role = np.int32(role)
    perm = rng.permutation(len(rig))
    rig, role = rig[perm], role[perm]
    # the cover of the world of 300 goes last of its world
    last = int(np.flatnonzero(rig["world"] == W300)[-1])
    cover = int(np.flatnonzero((rig["world"] == W300) & (role == COVER))[0])
    rig[[last, cover]], role[[last, cover]] = rig[[cover, last]], role[[cover, last]]
    assert np.bincount(rig["world"], minlength=len(scs)).tolist() == list(COUNTS)
    return rig, role


# ---- the boxes of mgf_batch_overlap_first_dev ---------------------------------------------------------------------------------------------
def fixed_boxes(scs, per, seed=98):
    """(boxes [K * per, 6], ignore [K * per]) in the fixed layout, box i for world i // per: the world's cover first, then cubes about
    body centres (about the origin in the world without bodies), every fifth lifted out of the pile; with per >= 3 a NaN box third;
    ignore: -1, a body of the world, or a value that names no body (the world's length, -7, INT32_MAX)"""
    rng = np.random.default_rng(seed + per)
    B, I = [], []
    for sc in scs:
        cen = SC.centres(sc)
        nb = len(cen)
        lo, hi = (cen.min(axis=0), cen.max(axis=0)) if nb else (np.zeros(3), np.ones(3))
        bx = np.empty((per, 6))
        at = cen[rng.integers(0, nb, per)] if nb else np.zeros((per, 3))
        bx[:, 0:3] = at + rng.normal(0.0, 0.4, (per, 3))
        bx[::5, 1] += 9.0
        bx[:, 3:6] = rng.uniform(0.2, 1.6, (per, 3))
        bx[0] = np.concatenate([(hi + lo) / 2, (hi - lo) / 2 + 2.0])
        if per >= 3:
            bx[2, 1] = np.nan
        ign = np.full(per, -1, np.int64)
        pick = rng.integers(0, 4, per)
        ign[pick == 1] = rng.integers(0, max(nb, 1), int(np.sum(pick == 1)))
        ign[pick == 2] = np.resize([nb, -7, (1 << 31) - 1], int(np.sum(pick == 2)))
        ign[0] = 0 if nb else 5                                       # the cover without body 0
        B.append(bx); I.append(ign)
    return np.concatenate(B).astype(f32), np.concatenate(I).astype(np.int32)


# ---- rigs for the plan alone --------------------------------------------------------------------------------------------------------------
PLAN_CASES = (("one", (1,)), ("three", (3,)), ("64", (64,)), ("65", (65,)), ("256", (256,)), ("257", (257,)),
              ("worlds that have none in between", (0, 3, 0, 257, 0, 0, 65, 0)))


def plan_worlds(counts, seed=99):
    """a world array with counts[k] zones for world k in one shuffled order"""
    w = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(counts)])
    return w[np.random.default_rng(seed).permutation(len(w))]
