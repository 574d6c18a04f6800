"""Shared by the tests of a batch's zones read nearest first (mgf_batch_read_zones_nearest / _read_zones_nearest_dev /
_overlap_nearest_dev), without a GPU: a numpy restatement of the definition in include/mgf_hip.h, f32 operation by operation -
    m = p (a sphere), p + d * 0.5 (a capsule)      e = m - c      d2 = (e.x * e.x + e.y * e.y) + e.z * e.z
the bodies of a zone's list in ascending (d2, body index), -1 and +inf behind them - written from the definition and not from the
kernel: the list itself is what overlap_boxes reports (tests/batch_zone_cases.py), the order is numpy's stable sort; and the tie scene,
a lattice on which whole shells of bodies are equally far, so that the index alone decides."""
import numpy as np

from tests import batch_zone_cases as ZC

f32 = np.float32
MAX_K = 32                          # MGF_BATCH_ZONE_NEAREST_MAX_K
KS = (0, 1, 8, 32)
INF_BITS = 0x7F800000


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def tight_centres(cols):
    """the centre of BoundedBy<AABB> of every collider (rows with tag, p, d: COMPONENT_DTYPE or MOVING_DTYPE): [n, 3] f32"""
    p, d = np.ascontiguousarray(cols["p"], f32).reshape(-1, 3), np.ascontiguousarray(cols["d"], f32).reshape(-1, 3)
    m = np.where((np.asarray(cols["tag"]) == 1)[:, None], p + d * f32(0.5), p)
    assert m.dtype == f32
    return m


def dist2(m, c):
    """d2 of centres m [j, 3] from the box centre c [3]: the three-step sum, every operation an f32 one"""
    e = np.ascontiguousarray(m, f32).reshape(-1, 3) - np.asarray(c, f32)
    sq = e * e
    out = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    assert out.dtype == f32
    return out


def record(lst, d2, k):
    """(1 + k int32 words, k f32 words) of a zone whose list (ascending body indices, self already removed) is lst, d2[j] of lst[j]"""
    lst, d2 = np.asarray(lst, np.int64), np.asarray(d2, f32)
    assert not np.any(np.isnan(d2)) and not np.any(np.signbit(d2))
    by = np.argsort(d2, kind="stable")[:k]        # lst ascends: a stable sort by d2 is the order by (d2, index)
    out, dd = np.full(1 + k, -1, np.int32), np.full(k, np.inf, f32)
    out[0] = len(lst)
    out[1:1 + len(by)] = lst[by]
    dd[:len(by)] = d2[by]
    return out, dd


def records(offsets, bodies, ignore, world, boxes, centres, lengths, k):
    """([n, 1 + k] int32, [n, k] f32) from the CSR lists of WorldBatch.overlap_boxes for `boxes` (rows c.xyz, r.xyz) against `world`,
    ignore[i] (-1: none) removed from list i; centres: tight_centres of the whole batch, worlds of `lengths` bodies concatenated"""
    n = len(offsets) - 1
    first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out, dd = np.empty((n, 1 + k), np.int32), np.empty((n, k), f32)
    for i in range(n):
        lst = np.asarray(bodies[int(offsets[i]):int(offsets[i + 1])], np.int64)
        lst = lst[lst != int(ignore[i])]
        out[i], dd[i] = record(lst, dist2(centres[first[int(world[i])] + lst], boxes[i, 0:3]), k)
    return out, dd


def brute_record(lst, d2, k):
    """the same record by Python's sort over (d2, index) pairs, d2 as exact Python floats"""
    pairs = sorted((float(x), int(i)) for x, i in zip(d2, lst))[:k]
    return [len(lst)] + [i for _, i in pairs] + [-1] * (k - len(pairs)), [x for x, _ in pairs] + [float("inf")] * (k - len(pairs))


# ---- the tie scene ------------------------------------------------------------------------------------------------------------------------
TIE_PITCH, TIE_CENTRE = 1.25, (0.0, 5.0, 0.0)
TIE_D2 = (0.0, 1.5625, 3.125, 4.6875)       # about the centre node: the node itself, 6 faces, 12 edges, 8 corners
TIE_SHELLS = (1, 6, 12, 8)
TIE_ZONE_R = 1.0                            # holds every tight box of the lattice: |dc| <= 1.25 <= 0.5 + 1.0 on every axis


def tie_scene(terrain, seed=41):
    """(scene, nodes [27, 3], centre body): 27 bodies of r = 0.5 on a 3 x 3 x 3 lattice of pitch 1.25 about TIE_CENTRE, in a shuffled
    body order; two bodies mirrored about the centre are short capsules along x whose tight box's centre is their node exactly
    (a = node - (0.25, 0, 0), d = (0.5, 0, 0): every operation exact).  Every coordinate is a small dyadic number: d2 is exact."""
    from mgf_amd import scenes
    g = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], np.float64)
    g = g[np.random.default_rng(seed).permutation(27)]
    nodes = (g * TIE_PITCH + np.float64(TIE_CENTRE)).astype(f32)
    comps = scenes._spheres(nodes, 0.5)
    a = int(np.flatnonzero(np.all(g == (1, 1, -1), axis=1))[0])
    b = int(np.flatnonzero(np.all(g == (-1, -1, 1), axis=1))[0])
    for i in (a, b):
        comps["tag"][i] = 1
        comps["d"][i] = (0.5, 0.0, 0.0)
        comps["p"][i] = nodes[i] - f32([0.25, 0.0, 0.0])
    sc = scenes._scene("tie_lattice", comps, terrain)
    return sc, nodes, int(np.flatnonzero(np.all(g == 0, axis=1))[0])


def tie_zones(world, centre_body):
    """ZONE_DTYPE rows: a zone fixed at the centre node; one on the centre body that lists it; one that ignores it"""
    from mgf_amd._capi import ZONE_DTYPE
    r = (TIE_ZONE_R,) * 3
    return np.array([(world, -1, TIE_CENTRE, r, 0, 0), (world, centre_body, (0.0, 0.0, 0.0), r, 0, 0),
                     (world, centre_body, (0.0, 0.0, 0.0), r, ZC.IGNORE_SELF, 0)], ZONE_DTYPE)


def scenes_and_rig():
    """(scenes, rig, role, tie): ZC.zone_scenes() with the tie world behind them, ZC.zone_rig() with the tie zones behind it (role -1);
    tie = (world, nodes, centre body, the rig rows of the tie zones)"""
    scs = ZC.zone_scenes()
    rig, role = ZC.zone_rig(scs)
    sc, nodes, centre = tie_scene(scs[0]["terrain"])
    w = len(scs)
    tz = tie_zones(w, centre)
    at = np.arange(len(rig), len(rig) + len(tz))
    return scs + [sc], np.concatenate([rig, tz]), np.concatenate([role, np.full(len(tz), -1, role.dtype)]), (w, nodes, centre, at)
