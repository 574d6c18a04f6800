"""Scenes and helpers for the batch's bodies of up to four components (mgf_batch_add_compound_bodies): tests/test_world_batch_parts_host.py
and tests/test_gpu_world_batch_parts.py.  Every world is 0 .. 64 bodies; the free runs are at most 150 ticks."""
import numpy as np

from mgf_amd import scenes
from tests import batch_obstacle_cases as BO
from tests.util import bits_equal, compare_constraints, oracle_world

f32 = np.float32
STATE = ("x", "q", "v", "omega", "delta")
COUNTS = ("n_constraints", "n_terrain_constraints", "n_pair_candidates", "n_refits")
TICKS = 150
LIST_TICKS = (1, 2, 10, 60, 150)
DUMBBELLS, JACKS, PILE, MIXED, EMPTY, ONE_JACK = range(6)


def n_bodies(sc):
    cb = sc.get("compound")
    return len(sc["comps"]) + (0 if cb is None else len(cb["offsets"]) - 1)


def merge_compound(a, b):
    """the "compound" block of a's bodies of several components followed by b's"""
    return dict(comps=np.concatenate([a["comps"], b["comps"]]), comp_mass=np.concatenate([a["comp_mass"], b["comp_mass"]]),
                offsets=np.concatenate([a["offsets"], b["offsets"][1:] + a["offsets"][-1]]).astype(np.int64),
                restitution=np.concatenate([a["restitution"], b["restitution"]]), friction=np.concatenate([a["friction"], b["friction"]]),
                force=np.concatenate([a["force"], b["force"]]))


def empty_scene(terrain):
    sc = scenes.sphere_pile(1, 1, 1)
    return dict(sc, name="empty", comps=sc["comps"][:0], mass=sc["mass"][:0], restitution=sc["restitution"][:0], friction=sc["friction"][:0],
                force=sc["force"][:0], v0=None, terrain=terrain)


def mixed_scene():
    """plain spheres, dumbbells and jacks in one world, as test_hip_worlds_mixing_one_two_and_four_parts builds it: the dumbbell scene
    lifted above the jacks, the jacks added behind it"""
    a, b = scenes.jack_field(3, 2, 3), scenes.dumbbell_field(3, 1, 3, n_plain=8)
    b["compound"]["comps"]["p"][:, 1] += f32(7.0)
    b["comps"]["p"][:, 1] += f32(9.0)
    sc = dict(b, name="mixed", compound=merge_compound(b["compound"], a["compound"]))
    sc["v0"] = np.concatenate([b["v0"], a["v0"]]).astype(f32)
    return sc


def six_scenes():
    """0 dumbbells and four plain spheres, 1 jacks, 2 a pile of plain spheres, 3 one, two and four parts mixed, 4 no bodies, 5 one jack - each
    over its own terrain"""
    d = scenes.dumbbell_field(3, 2, 3, n_plain=4)
    return [d, scenes.jack_field(3, 2, 3), scenes.sphere_pile(4, 6, 4, seed=5), mixed_scene(), empty_scene(d["terrain"]), scenes.jack_field(1, 1, 1)]


def obstacle_scenes():
    """the jacks over [ramp0, ring0], the dumbbells over the two in the other order, eight jacks without terrain over the ring"""
    o = BO.obstacle_scenes()
    ramp0, ring0 = o[BO.BOX]["obstacles"]
    ring_low = o[BO.BARE]["obstacles"][0]
    return [dict(scenes.jack_field(3, 2, 3), obstacles=[ramp0, ring0]), dict(scenes.dumbbell_field(3, 2, 3, n_plain=4), obstacles=[ring0, ramp0]),
            dict(scenes.jack_field(2, 2, 2), terrain=None, obstacles=[ring_low])]


def largest_manifold(cons):
    """the longest run of consecutive records of one pair of bodies in a constraint list"""
    best = run = 0
    for k in range(len(cons)):
        same = k > 0 and cons["b"][k] >= 0 and cons["a"][k] == cons["a"][k - 1] and cons["b"][k] == cons["b"][k - 1]
        run = run + 1 if same else (1 if cons["b"][k] >= 0 else 0)
        best = max(best, run)
    return best


def same_state(got, want, what):
    for f in STATE:
        assert bits_equal(got[f], want[f]), f"{what}: {f} differs"


def same_counts(st, ost, what):
    for f in COUNTS:
        assert getattr(st, f) == getattr(ost, f), f"{what}: {f} = {getattr(st, f)}, the reference has {getattr(ost, f)}"


def run_against_oracle(b, ows, scs, ticks, list_ticks):
    """the batch free running beside one oracle world per scene, state bits and counts every tick, the list with impulses on list_ticks;
    returns per world (most constraints, most terrain contacts, terrain contacts summed, largest manifold) from the oracle's own lists"""
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    seen = [[0, 0, 0, 0] for _ in scs]
    for tick in range(1, ticks + 1):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k} tick {tick}"
            assert st[k].n_bodies == n_bodies(scs[k]) and st[k].iters == iters, what
            same_counts(st[k], ost, what)
            same_state(b.state(k), ow.state(), what)
            oc = ow.constraints()
            if tick in list_ticks:
                compare_constraints(b.constraints(k), oc, check_impulse=True)
            s = seen[k]
            s[0] = max(s[0], int(ost.n_constraints)); s[1] = max(s[1], int(ost.n_terrain_constraints)); s[2] += int(ost.n_terrain_constraints)
            s[3] = max(s[3], largest_manifold(oc))
    return seen


def fill_world(b, k, sc):
    """the bodies of a scene into world k, as WorldBatch.from_scenes adds them"""
    if len(sc["comps"]):
        b.add_bodies(k, sc["comps"], sc["mass"], sc["restitution"], sc["friction"], sc["force"])
    cb = sc.get("compound")
    if cb is not None:
        b.add_compound_bodies(k, cb["comps"], cb["comp_mass"], cb["offsets"], cb["restitution"], cb["friction"], cb["force"])
    if sc.get("v0") is not None and b.world_len(k):
        b.write_state(k, v=sc["v0"])


def oracles(scs):
    return [BO.oracle_with_obstacles(sc) if sc.get("obstacles") is not None else oracle_world(sc) for sc in scs]
