"""Scenes of wide bodies that meet each other, and the CPU side of their checks (WideSpec in k_bodies.h, k_pair_wide in k_front_rows.h).

A wide body is kept out of the scene's rmax, the reach of the cell grid's queries.  Pair (i, j) - j the body of the smaller order id - is
accepted when i's tight (swept) box overlaps j's fat box (bvh.rs:297, world.rs:266).  If both are wide, i's centre can lie far outside
fat_j grown by rmax while its tight box still meets fat_j: two runaways flying at each other, or a fast one catching a slower one.  The
scenes here put such a pair into exactly that region at a chosen tick, and `lost_region_checks` proves it from the oracle's own boxes."""
import numpy as np

from mgf_amd import scenes
from tests.util import oracle_world

FAT_MARGIN = 0.25  # world.rs:181,237
MEET_TICK = 6      # the tick (0-based) in which the scripted pairs touch
FAR_Y = -2500.0    # far below every scene: the pair is alone there
FUZZ_SEED_BASE = 10000  # fuzz_scene's seed for seed k of tools/wide_pairs_fuzz.py
KINDS = ("spheres", "capsules", "capsule_vs_sphere", "two_part_bodies", "sixteen_part_bodies")


def base_scene(kind):
    """the world the runaways are taken from, and the bodies that may run away (single-component ones: a kind's plain spheres)"""
    if kind == "spheres":
        sc = scenes.sphere_pile(12, 12, 12)
    elif kind in ("capsules", "capsule_vs_sphere"):
        sc = scenes.capsule_field(8, 6, 8, quads=12, pitch=1.6)
    elif kind == "two_part_bodies":
        sc = scenes.dumbbell_field(6, 4, 6, n_plain=40)
    elif kind == "sixteen_part_bodies":
        sc = scenes.caterpillar_field(4, 2, 4, n_plain=30)
    else:
        raise ValueError(kind)
    return sc


def place(scene, movers):
    """the scene with some of its single-component bodies moved, re-shaped and thrown: [(body, centre, velocity, shape)], shape
    ("sphere", r) or ("capsule", r, half length, tilt): a capsule in the x-y plane, turned by `tilt` degrees from the x axis"""
    sc = dict(scene)
    comps, v0 = scene["comps"].copy(), scene["v0"].copy()
    for body, c, vel, shape in movers:
        c = np.asarray(c, np.float32)
        if shape[0] == "sphere":
            comps["tag"][body] = 0
            comps["p"][body] = c
            comps["d"][body] = np.float32(0.0)
            comps["r"][body] = np.float32(shape[1])
        else:
            t = np.radians(shape[3])
            d = np.float32([2.0 * shape[2] * np.cos(t), 2.0 * shape[2] * np.sin(t), 0.0])
            comps["tag"][body] = 1
            comps["p"][body] = c - d * np.float32(0.5)
            comps["d"][body] = d
            comps["r"][body] = np.float32(shape[1])
        v0[body] = np.asarray(vel, np.float32)
    sc["comps"], sc["v0"] = comps, v0
    return sc


def _reach(shape):
    """how far the shape reaches along x from its centre, and the height of that tip above the centre"""
    if shape[0] == "sphere":
        return shape[1], 0.0
    t = np.radians(shape[3])
    return shape[1] + shape[2] * np.cos(t), shape[2] * abs(np.sin(t))


# per kind: head-on speeds, catch-up speeds, the crossing catch-up's speeds (see meeting_scene), and how far past fat_j + rmax i's centre has to
# lie: more than a cell of the grid, or the cell walk reaches i's cell all the same (the fields of bodies of several parts are few bodies
# with large rest extents - coarse cells, a large rmax and a high limit of "wide": faster runaways there)
_PLAN = {"spheres": ((240.0, 200.0), (420.0, 110.0), (600.0, 110.0, 480.0), 0.9),
         "capsules": ((280.0, 240.0), (420.0, 110.0), (600.0, 110.0, 540.0), 0.9),
         "two_part_bodies": ((540.0, 450.0), (860.0, 200.0), (900.0, 200.0, 730.0), 2.0),
         "sixteen_part_bodies": ((1000.0, 850.0), (1800.0, 500.0), (1500.0, 500.0, 1300.0), 3.0)}
_PLAN["capsule_vs_sphere"] = _PLAN["capsules"]


def min_margin(kind):
    return _PLAN[kind][3]


def meeting_scene(kind, motion, fast_larger):
    """Two runaways near y = FAR_Y that touch in tick MEET_TICK while i's centre lies more than min_margin(kind) further from fat_j's
    than fat_j + rmax reaches, along x or z (far below the grid the cells' y clamps: a pair apart along y shares their bottom row).
    motion "head_on": two bodies at each other along x (240 and 200 m/s in the pile).  "catch_up": a fast body overtakes a slower one along x.  With the slower one as i,
    a tight box that reaches fat_j from outside fat_j + rmax along x would need a radius that itself raises the limit of "wide": there the
    slower one also crosses the fast one's line along z, and the pair is lost along z.  fast_larger: the faster body has the larger order
    id.  Capsules lie in the x-y plane, the left one turned by +10 degrees and the right one by -10, so that their tips meet (the oracle
    finds two capsules on ONE line a tick late).  -> (scene, (i, j)): i the body of the larger order id."""
    sc = base_scene(kind)
    dt = float(sc["dt"])
    n = len(sc["comps"])
    lo, hi = (7, n - 5) if kind in ("spheres", "capsules", "capsule_vs_sphere") else (1, n - 2)  # (single-component bodies come first)
    fast_b, slow_b = (hi, lo) if fast_larger else (lo, hi)
    head_on, catch_up, crossing, _ = _PLAN[kind]
    capsules = kind in ("capsules", "capsule_vs_sphere")
    left = ("capsule", 0.25, 0.5, 10.0) if capsules else ("sphere", 0.5)  # the fast body, on the left, moving +x
    right = ("capsule", 0.25, 0.5, -10.0) if kind == "capsules" else ("sphere", 0.5)
    m = MEET_TICK
    if motion == "catch_up" and not fast_larger:
        # two spheres: the slower one (vx, 0, -vz) crosses z from +sz/2 to -sz/2 in the tick, the fast one runs along x at z = -sz/2; at
        # time t of the tick both centres share x and are 0.5 apart in z (less than the radii's sum: they touched by then)
        vf, vx, vz = crossing
        sf, sx, sz = vf * dt, vx * dt, vz * dt
        t = 1.0 - 0.5 / sz
        movers = [(fast_b, (-m * sf, FAR_Y, -0.5 * sz), (vf, 0.0, 0.0), ("sphere", 0.5)),
                  (slow_b, ((sf - sx) * t - m * sx, FAR_Y, 0.5 * sz + m * sz), (vx, 0.0, -vz), ("sphere", 0.5))]
        return place(sc, movers), (hi, lo)
    vf, vs = head_on if motion == "head_on" else catch_up
    sf, ss = vf * dt, vs * dt
    (ef, hf), (es, hs) = _reach(left), _reach(right)
    # the gap between the centres at the start of the meeting tick: 0.15 m closer than the largest gap the tick's motion closes
    if motion == "head_on":
        g = ef + es + sf + ss - 0.15
        uf, us = vf, -vs
    else:
        g = ef + es + sf - ss - 0.15
        uf, us = vf, vs
    z = 0.3
    movers = [(fast_b, (-0.5 * g - m * uf * dt, FAR_Y - hf, z), (uf, 0.0, 0.0), left),
              (slow_b, (0.5 * g - m * us * dt, FAR_Y - hs, z), (us, 0.0, 0.0), right)]
    return place(sc, movers), (hi, lo)


def fuzz_scene(seed, base="spheres"):
    """2..40 runaways taken from a 12^3 pile ("spheres") or a small field of two-part bodies ("two_part_bodies"): some on a shell outside the
    bounds, some inside, 50..600 m/s, about a third aimed at another runaway -> (scene, the runaways' bodies)"""
    rng = np.random.default_rng(seed)
    sc = scenes.sphere_pile(12, 12, 12) if base == "spheres" else scenes.dumbbell_field(5, 3, 5, n_plain=60)
    n_single = len(sc["comps"])
    k = int(rng.integers(2, 41 if base == "spheres" else min(41, n_single)))
    bodies = rng.choice(n_single, size=k, replace=False)
    p = sc["comps"]["p"]
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pos = np.empty((k, 3))
    for a in range(k):
        if rng.random() < 0.5:  # a shell outside the bounds
            u = rng.normal(size=3)
            pos[a] = centre + u / np.linalg.norm(u) * rng.uniform(1.2, 3.0) * np.linalg.norm(half)
        else:
            pos[a] = rng.uniform(lo, hi)
    vel = np.empty((k, 3))
    for a in range(k):
        speed = rng.uniform(50.0, 600.0)
        if k > 1 and rng.random() < 1.0 / 3.0:  # aimed at another runaway
            b = int(rng.integers(0, k - 1))
            b += b >= a
            u = pos[b] - pos[a]
        else:
            u = rng.normal(size=3)
        vel[a] = u / max(np.linalg.norm(u), 1e-6) * speed
    movers = [(int(bodies[a]), pos[a], vel[a], ("sphere", float(sc["comps"]["r"][bodies[a]]))) for a in range(k)]
    return place(sc, movers), [int(b) for b in bodies]


def tight_boxes(ow):
    """every single-component body's swept box as the oracle forms it (bounds of Moving<Component>: the shape's box combined with the
    box moved by delta, collision.rs / bounds.rs), in f32: (centres, half extents)"""
    comps, d = ow.colliders()
    f = np.float32
    p, dd, r = comps["p"].astype(f), comps["d"].astype(f), comps["r"].astype(f)
    cap = comps["tag"] == 1
    mag = np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
    rr = np.where(cap, r + mag * f(0.5), r).astype(f)
    c = np.where(cap[:, None], p + dd * f(0.5), p).astype(f)
    sr = np.repeat(rr[:, None], 3, axis=1)
    e = c + d.astype(f)
    lower = np.minimum(c - sr, e - sr)
    upper = np.maximum(c + sr, e + sr)
    return ((upper + lower) / f(2.0)).astype(f), ((upper - lower) / f(2.0)).astype(f)


def fat_boxes(ow):
    """every body's fat box as it sits in the oracle's world BVH: (centres, half extents) by body index"""
    nodes, b = ow.world_bvh().dump()
    leaf = (nodes[:, 0] == 1) & (nodes[:, 3] == 1)
    ids = nodes[leaf, 4]
    n = len(ow)
    c, r = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
    c[ids], r[ids] = b[leaf, :3], b[leaf, 3:]
    assert not np.isnan(c).any(), "a body without a leaf in the world BVH"
    return c, r


def overlaps(ac, ar, bc, br):
    """collision.rs:22-29 in f32, broadcasting"""
    return np.all(np.abs(ac - bc) <= ar + br, axis=-1)


def accepted_pairs(tc, tr, fc, fr, single):
    """every (i, j), j < i, whose tight box of i meets the fat box of j, by brute force; `single`: the bodies whose tight box
    tight_boxes knows (all of them in a world of single-component bodies) -> set of (i, j)"""
    out = set()
    idx = np.flatnonzero(single)
    for i in idx[idx > 0]:
        hit = np.flatnonzero(overlaps(tc[i][None, :], tr[i][None, :], fc[:i], fr[:i]))
        out.update((int(i), int(j)) for j in hit)
    return out


def lost_region_checks(ow, i, j, runaways, margin=0.0):
    """After the oracle's build_constraints of the meeting tick: i's tight box meets fat_j, and both i's tight-box centre and its fat-box
    centre lie more than `margin` outside fat_j grown by rmax (the largest fat half extent of the bodies that are not runaways) along x or
    z - the region the cell walk of k_pair_wide searched - and the oracle holds a constraint between i and j.  Returns a line for the
    failure message."""
    tc, tr = tight_boxes(ow)
    fc, fr = fat_boxes(ow)
    keep = np.ones(len(ow), bool)
    keep[list(runaways)] = False
    rmax = fr[keep].max(axis=0)
    reach = fr[j] + rmax
    xz = [0, 2]
    assert overlaps(tc[i], tr[i], fc[j], fr[j]), f"tight_{i} {tc[i]} +- {tr[i]} misses fat_{j} {fc[j]} +- {fr[j]}"
    assert np.any((np.abs(tc[i] - fc[j]) - reach)[xz] > margin), f"tight_{i}'s centre {tc[i]} lies within fat_{j} {fc[j]} +- {reach} + {margin}"
    assert np.any((np.abs(fc[i] - fc[j]) - reach)[xz] > margin), f"fat_{i}'s centre {fc[i]} lies within fat_{j} {fc[j]} +- {reach} + {margin}"
    cons = ow.constraints()
    assert np.any((cons["a"] == i) & (cons["b"] == j)), f"no constraint between {i} and {j} in the oracle's meeting tick"
    return f"|c_i - c_j| {np.abs(fc[i] - fc[j])}, fat_j + rmax {reach}, rmax {rmax}"
