"""Shared by the tests of a rollout's sensor trace (mgf_batch_rollout_observe / _rollout_observe_dev; WorldBatch.rollout_observe /
.rollout_observe_dev), without a GPU: ray-sensor rigs for the scenes of tests/batch_rollout_cases.py - the late-contact pair, whose
spheres close in on each other and on the floor, so that what a body-mounted ray meets changes from tick to tick - and for a pair of
worlds of tests/batch_obstacle_cases.py, one with obstacles and one without; and what the ORACLE says the late rig sees tick by tick,
which tests/test_world_batch_scan_host.py holds to the condition the GPU test needs: a row written from the wrong tick shows."""
import functools

import numpy as np

from mgf_amd._capi import SENSOR_DTYPE
from tests import batch_obstacle_cases as BC
from tests import batch_rollout_cases as RC
from tests import batch_sensor_cases as SC
from tests import batch_trace_cases as XC
from tests.util import oracle_world

f32 = np.float32
T = XC.T                             # ticks of the late-contact rollouts: both capacity re-runs in the middle of the call
PER_BODY = (10, 3, 2)                # sensors a body of LATE_A, LATE_B, SPARSE: 270 on LATE_A - one world, two work items
HIT_NONE, HIT_BODY, HIT_TERRAIN, HIT_OBSTACLE = -1, 0, 1, 2


# ---- the late-contact pair ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _late_rig(seed=171):
    scs = RC.late_contact_scenes()
    rng = np.random.default_rng(seed)
    rows = []
    for k, (sc, per) in enumerate(zip(scs, PER_BODY)):
        n = len(sc["comps"])
        centre = sc["comps"]["p"].astype(np.float64)
        foot = np.array([0.0, 0.5, 0.0])
        for bd in range(n):
            for j in range(per):
                s = np.zeros(1, SENSOR_DTYPE)
                s["world"], s["body"] = k, bd
                if j == 0:
                    d = np.array([0.0, -1.0, 0.0])                   # the floor below, or the sphere below
                elif j == 1:
                    d = foot - centre[bd]                             # where every sphere of a lattice is heading
                    d = d / np.linalg.norm(d) if np.linalg.norm(d) > 1e-6 else np.array([1.0, 0.0, 0.0])
                else:
                    d = rng.normal(0, 1, 3)
                    d /= np.linalg.norm(d)
                d = d * rng.uniform(0.5, 2.0)                         # (t is in units of |d|)
                seen = j % 3 == 2                                      # a third may see their own body, and start outside it
                s["p"] = 0.6 * d / np.linalg.norm(d) if seen else 0.0
                s["d"] = d
                s["dt"] = np.inf if j % 2 == 0 else 8.0
                s["flags"] = 0 if seen else SC.IGNORE_SELF
                rows.append(s)
    rig = np.concatenate(rows)
    return np.ascontiguousarray(rig[rng.permutation(len(rig))])


def late_sensor_rig():
    """the ray sensors of RC.late_contact_scenes(): PER_BODY on every body of the three worlds - straight down, at the lattice's foot,
    any way; every second one a segment, a third without IGNORE_SELF from just outside their body - in one seeded shuffle: a copy"""
    return _late_rig().copy()


def sphere_hits(rig, state, lengths, radius=0.5):
    """(kind, index, t) of every sensor against the SPHERES of its world alone, by the oracle's Intersects<Sphere> and the definition's
    particles (SC.rig_particles): the nearest t, the lowest index among equals.  No terrain: what the bodies alone show."""
    from oracle import oracle as O
    P, D, dt = SC.rig_particles(rig, state, lengths)
    off = SC.offsets(lengths)
    ign = SC.ignore_of(rig)
    out = np.zeros(len(rig), np.dtype([("kind", "<i4"), ("index", "<i4"), ("t", "<f4")]))
    out["kind"] = HIT_NONE
    for i in range(len(rig)):
        k = int(rig["world"][i])
        best = None
        for j in range(lengths[k]):
            if j == ign[i]:
                continue
            hit = O.intersection(P[i], D[i], float(dt[i]), O.shape(O.SPHERE, state["x"][off[k] + j], radius))
            if hit is not None and (best is None or hit[1] < best[1]):
                best = (j, hit[1])
        if best is not None:
            out[i] = (HIT_BODY, best[0], best[1])
    return out


@functools.lru_cache(maxsize=None)
def _late_oracle():
    scs = RC.late_contact_scenes()
    ows = [oracle_world(sc) for sc in scs]
    lengths = [len(sc["comps"]) for sc in scs]
    rig = _late_rig()
    counts, seen = [], []
    for _ in range(T):
        for sc, ow in zip(scs, ows):
            ow.step(float(sc["dt"]), sc["iters"])
        st = [ow.state() for ow in ows]
        state = {key: np.concatenate([s[key] for s in st]) for key in ("x", "q")}
        counts.append([len(ow.constraints()) for ow in ows])
        seen.append(sphere_hits(rig, state, lengths))
    return np.array(counts), np.stack(seen)


def late_oracle_view():
    """(counts[t][k], seen[t][i]): the oracle's constraints per tick and world, no actuator acting, and sphere_hits of the late rig
    behind every tick; not to be written to"""
    return _late_oracle()


# ---- a world with obstacles beside one without --------------------------------------------------------------------------------------------
def obstacle_pair():
    """world 0 of BC.obstacle_scenes() with its ring listed first (SC.ring_of aims at the first entry) and its ramp, and world 4: the
    same pile without obstacles"""
    o = BC.obstacle_scenes()
    return [dict(o[0], obstacles=list(o[0]["obstacles"][::-1])), o[4]]


def obstacle_layout(scs):
    """on the world with obstacles 12 sensors at the ring from above, 6 down, 6 up, the special ones and 20 any way; 16 on the other"""
    lay = SC._layout(scs, [dict(n_random=28, n_down=6, n_up=6, n_ring=12, special=True), dict(n_random=12, n_down=4)], seed=173)
    assert np.bincount(lay["world"], minlength=2).tolist() == [52, 16]
    return lay


def depth_of(hits, rig):
    """the MGF_ROLLOUT_SENSOR_DEPTH rows of MGF_ROLLOUT_SENSOR_HIT ones: the hit's t, the sensor's dt where nothing is hit"""
    return np.where(hits["kind"] == HIT_NONE, rig["dt"].astype(f32)[None, :], hits["t"]).astype(f32)
